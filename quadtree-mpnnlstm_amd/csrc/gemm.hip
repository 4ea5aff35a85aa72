// The dense products of the library.  qt_gemm.h holds the operands and the argument block, and the one copy of what these kernels
// share: the epilogue activation (act_quad, relu_bwd_quad), the 4 x 4 FMA block (fma_quad, post_product), the split store
// (store_split) and the staged epilogue of the three MFMA kernels (stage_and_store).
//   k_gemm_fwd -- fp32 MFMA (32x32x2) GEMM: Y = [T_0 .. T_{K-1} | S] W of the Chebyshev planes and the data gradients; with CELL,
//              the gate GEMM that runs the LSTM cell in its epilogue (launched for gatecell.hip by gemm_fwd_cell_launch)
//   k_gemm_skinny / k_gemm_row16 / k_head_dgrad -- few output columns or a short reduction (the decoder head), on the VALU
//   k_gemm_fwd3 / k_gemm_sb -- bf16x3 and split-bf16 variants
//   k_gemm_wgrad / k_gemm_wgrad_group -- the weight gradient split over row blocks;  k_colsum -- fixed-order sum of the blocks
#include "qt_cell.h"
#include "qt_gemm.h"
#include <cstdlib>

namespace {

// MODE 0: out planes = act(A @ W).  Block = 128 node rows x (32 NT) output columns, wave w owns rows [32w, 32w+32).
// A fragments go global -> VGPR directly (float4 per lane and k-quad); only W is staged in LDS (KWT x 32 NT floats).
// NT = 2 for NB <= 64 (gate GEMM), NT = 4 for wide outputs (the data gradient, NB = K*C) so A is read only once.
static constexpr int QT_GEMM_OCC = 4;
static constexpr int QT_GEMM_OCC3 = 3;
static constexpr int QT_GEMM_OCC4C = 2;
// CELL: 0 = plain epilogue, else the lanes per node (h / 4) of the fused LSTM cell.  Workgroups per CU: 4, so that all N/128
// blocks of the bench shape are resident at once (<= 128 registers); 3 for NT = 3 and 2 for the NT = 4 cell epilogue.
template <int NT, int KWT, int CELL = 0>
__global__ __launch_bounds__(256, (NT == 4 && CELL != 0) ? QT_GEMM_OCC4C : (NT == 3 ? QT_GEMM_OCC3 : QT_GEMM_OCC)) void k_gemm_fwd(GemmArgs g) {
    constexpr int BNT = 32 * NT;
    constexpr int PITCH = KWT + 4;      // == 4 (mod 64) floats: the 16 lanes of a ds_read_b128 group hit distinct banks
    // W chunk TRANSPOSED in LDS, Bt[column][k]: a lane's four B operands of one k-quad are one ds_read_b128
    // (measured: with one ds_read_b32 per MFMA the kernel ran at half the MFMA rate)
    __shared__ __attribute__((aligned(16))) float Bt[BNT * PITCH];
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int j0 = blockIdx.y * BNT;
    const int64_t rows = qt_rows(g.n_dev, g.M);      // g.M stays the plane stride (capacity)
    if (i0 >= rows) return;
    if (gridDim.z > 1) {
        const int z = g.zrev ? (int)gridDim.z - 1 - (int)blockIdx.z : (int)blockIdx.z;     // (zrev: groups from the last to the first)
        g.A.a0 += z * g.gsA;
        if (g.A.a_rest) g.A.a_rest += z * g.gsA;
        if (g.B) g.B += z * g.gsB;
        if (g.BT) g.BT += z * g.gsB;
        g.out += z * g.gsO;
    }
    const int nquad = g.K >> 2;
    build_quad_table(g.A, qptr, qstr, nquad);
    const int64_t my_row = i0 + wave * 32 + l32;
    const bool row_ok = my_row < rows;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    // fused cell: this thread's previous cell states (one node per epilogue pass) are requested now, before the MFMA loop,
    // so the epilogue does not start with a dependent memory round trip
    constexpr int NPASS = CELL != 0 ? BM / (256 / (CELL != 0 ? CELL : 1)) : 1;
    float4 cpre[NPASS];
    if constexpr (CELL != 0) {
#pragma unroll
        for (int ps = 0; ps < NPASS; ++ps) {
            const int64_t node = i0 + ps * (256 / CELL) + t / CELL;
            cpre[ps] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (node < rows && g.Cprev) cpre[ps] = *reinterpret_cast<const float4*>(g.Cprev + node * g.ld_c + (t % CELL) * 4);
        }
    }
    for (int k0 = 0; k0 < g.K; k0 += KWT) {
        const int kn = min(KWT, g.K - k0);           // multiple of 4
        __syncthreads();                              // table ready / previous pass done with Bs
        // W chunk -> LDS first (small, L2 resident) ...
        if (g.BT) {
            // ... from W^T: a column's k run is contiguous in memory and in LDS (conflict-free 16-byte stores)
            const int kqn = kn >> 2;
            for (int e = t; e < BNT * kqn; e += 256) {
                const int c = e / kqn, kq = e - c * kqn;
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j0 + c < g.NB) w = *reinterpret_cast<const float4*>(g.BT + (int64_t)(j0 + c) * g.K + k0 + 4 * kq);
                *reinterpret_cast<float4*>(&Bt[c * PITCH + 4 * kq]) = w;
            }
        } else {
            for (int e = t; e < kn * (BNT / 4); e += 256) {
                const int kb = e / (BNT / 4), jq = (e % (BNT / 4)) * 4;
                float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
                if (j0 + jq < g.NB) w = *reinterpret_cast<const float4*>(g.B + (int64_t)(k0 + kb) * g.NB + j0 + jq);
                Bt[(jq + 0) * PITCH + kb] = w.x;
                Bt[(jq + 1) * PITCH + kb] = w.y;
                Bt[(jq + 2) * PITCH + kb] = w.z;
                Bt[(jq + 3) * PITCH + kb] = w.w;
            }
        }
        for (int e = t; e < BNT * ((KWT - kn) / 4); e += 256) {          // zero the k tail of a short last pass
            const int c = e / ((KWT - kn) / 4), kq = kn + (e % ((KWT - kn) / 4)) * 4;
            *reinterpret_cast<float4*>(&Bt[c * PITCH + kq]) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        // ... then the MFMA stream.  The A quads (quad 2 j + half of this lane's row) come straight from global memory
        // through a 4-deep register ring loaded four k-groups ahead; the loop is a plain runtime loop with NO branch
        // around the MFMAs (conditionals there made hipcc shuttle the accumulators between VGPRs and AGPRs: 1088
        // v_accvgpr moves and a vmcnt(0) per group, 2.75x slower than the MFMA rate).
        const int q0 = k0 >> 2, qn = kn >> 2, nj = (kn + 7) >> 3;
        auto ldq = [&](int j) {
            const int q = 2 * j + half;
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row_ok && q < qn) r = gload4(qptr[q0 + q] + my_row * qstr[q0 + q]);
            return r;
        };
        float4 a0 = ldq(0), a1 = ldq(1), a2 = ldq(2), a3 = ldq(3);
        for (int j = 0; j < nj; ++j) {
            const float4 a = a0;
            a0 = a1; a1 = a2; a2 = a3;
            a3 = ldq(j + 4);
            float4 bq[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                bq[nt] = *reinterpret_cast<const float4*>(&Bt[(nt * 32 + l32) * PITCH + 8 * j + 4 * half]);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {      // (mfma_quad's text: through the helper four register moves of the ring shift change place)
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq[nt].x, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq[nt].y, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq[nt].z, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq[nt].w, acc[nt], 0, 0, 0);
            }
        }
    }
    float* Cs = Bt;                              // 128 rows x 64 columns per pass
    if constexpr (CELL != 0) {
        // LSTM epilogue: h / 4 adjacent lanes own a node, as in k_lstm_fwd (h = 8, 16 with NT = 2; h = 32 with NT = 4: all
        // four gates of a node sit in this block's 32 NT columns).  The gate tile goes through LDS 256 / (h/4) rows at a
        // time with a row pitch of 5 h floats: the rows a 16-lane ds_read_b128 phase touches then start h banks apart.
        // Same arithmetic, in the same order, as qt_dense followed by qt_lstm_fwd.
        using namespace qtcell;
        __builtin_assume(g.gates != nullptr);    // (qt_dense_lstm refuses a launch without them: store_cell's test folds away)
        constexpr int lpn = CELL;                // 2, 4 or 8 lanes per node
        constexpr int h = 4 * lpn;
        constexpr int CP = 5 * h;
        constexpr int RP = 256 / lpn;            // rows per pass: 128, 64 or 32
        static_assert(4 * h <= 32 * NT && BNT * PITCH >= RP * CP, "gate tile does not fit");
#pragma unroll
        for (int r0 = 0; r0 < BM; r0 += RP) {
            __syncthreads();
            if (wave * 32 >= r0 && wave * 32 < r0 + RP) {
#pragma unroll
                for (int u = 0; u < NT; ++u)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (u * 32 < 4 * h)      // (h = 8: the second 32-column tile is padding)
                            Cs[(wave * 32 - r0 + acc_row(r, half)) * CP + u * 32 + l32] = acc[u][r];
            }
            __syncthreads();
            const int row = t / lpn, j0 = (t - row * lpn) * 4;
            const int64_t node = i0 + r0 + row;
            const bool ok = node < rows;
            F4 gi, gf, gc, go;
            ld_gates(Cs + row * CP + j0, h, &gi, &gf, &gc, &go);
            const float4 c4 = cpre[r0 / RP];
            const F4 cp = {{c4.x, c4.y, c4.z, c4.w}};
            const CellOut r = cell_forward<lpn>(gi, gf, gc, go, cp, g.wc, g.bias, g.ln, h, j0);
            if (ok) store_cell(g.O, g.Hn, g.Cn, g.gates, node, h, j0, r);
        }
        return;
    }
    static_assert(BNT * PITCH >= BM * 64, "LDS staging tile does not fit in the W buffer");
    stage_and_store<NT>(acc, Cs, g, i0, j0, rows);
}

// ---- skinny shapes: few output columns (the decoder head: 16 or 4) or a short reduction (its data gradients: K = 16 or 4).
// The MFMA kernel's fixed costs (W staging, barriers, the LDS round trip of the epilogue: ~15 us) dwarf such a product; here a
// wave owns 64 rows x 4 output columns, reads its A quads straight from global memory and the matching 4 x 4 block of W
// through scalar loads (wave uniform), and accumulates with plain fp32 FMAs -- the VALU has the fp32 MFMA's FLOP rate.
// RPB = 64: the 4 waves of a workgroup take 4 column quads of the same 64 rows (their A loads meet in L1); RPB = 256: one
// column quad in all (NB = 4).
static constexpr int QT_SKINNY_INFLIGHT = 4;      // A quads in flight per trip (8: +0.02 ms per step, 16: +0.07)
template <int RPB>
__global__ __launch_bounds__(256) void k_gemm_skinny(GemmArgs g) {
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    __shared__ float hs[RPB == 64 ? 64 * 17 : 1];       // (post product: the 64 x 16 output tile, pitch 17)
    const int t = threadIdx.x;
    const int64_t rows = qt_rows(g.n_dev, g.M);
    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    if (row0 >= rows) return;
    const int nquad = g.K >> 2;
    build_quad_table(g.A, qptr, qstr, nquad);
    __syncthreads();
    const int cq = __builtin_amdgcn_readfirstlane(RPB == 64 ? (int)blockIdx.y * 4 + (t >> 6) : (int)blockIdx.y);
    const int j = cq * 4;
    if (j >= g.NB) return;
    const int64_t row = row0 + (RPB == 64 ? (t & 63) : t);
    const bool ok = row < rows;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* __restrict__ Wc = g.B + j;
    auto lda = [&](int Q) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && Q < nquad) r = gload4(qptr[Q] + row * qstr[Q]);
        return r;
    };
    for (int Q = 0; Q < nquad; Q += QT_SKINNY_INFLIGHT) {            // A quads in flight per trip (a trip is one dependent memory phase)
        float4 aq[QT_SKINNY_INFLIGHT];
#pragma unroll
        for (int u = 0; u < QT_SKINNY_INFLIGHT; ++u) aq[u] = lda(Q + u);
#pragma unroll
        for (int u = 0; u < QT_SKINNY_INFLIGHT; ++u)
            if (Q + u < nquad) fma_quad(acc, aq[u], Wc + (int64_t)4 * (Q + u) * g.NB, g.NB);
    }
    const bool post = RPB == 64 && g.post_W != nullptr;       // (uniform; the host guarantees NB == 16: all four waves are here)
    if (!ok && !post) return;
    float4 v = acc;
    if (g.act == QT_ACT_RELU) v = act_quad(v, QT_ACT_RELU, (g.drop && ok) ? g.drop[row] : 1.0f, 0.0f);
    if (g.act == QT_ACT_RELU_BWD && ok)            // G = v * relu'(Y): k_act_bwd's arithmetic, Y = g.res (M, res_stride)
        v = relu_bwd_quad(v, *reinterpret_cast<const float4*>(g.res + row * g.res_stride + j));
    if constexpr (RPB == 64) {
        if (post) {
            // the second product, by wave 0 from the tile in LDS
            float* h = &hs[(t & 63) * 17 + j];
            h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
            __syncthreads();
            if (t < 64 && ok) {
                const float* r = &hs[t * 17];
                const float4 q[4] = {make_float4(r[0], r[1], r[2], r[3]), make_float4(r[4], r[5], r[6], r[7]),
                                     make_float4(r[8], r[9], r[10], r[11]), make_float4(r[12], r[13], r[14], r[15])};
                *reinterpret_cast<float4*>(g.post_out + row * 4) = post_product(q, g.post_W);
            }
            if (!ok) return;
        }
    }
    if (g.act == QT_ACT_TANH_RES) v = act_quad(v, QT_ACT_TANH_RES, g.drop ? g.drop[row] : 1.0f, g.res[row * g.res_stride]);
    store_split(g, j, row, v, g.Cb);
}

// ---- one lane = one node row, ALL 16 output columns: the decoder head's products (fc_out1: 20 -> 16 channels over K = 3 planes,
// model/seq2seq.py:115-121,164-171).  k_gemm_skinny<64> gives a wave 4 of the 16 columns, so the four waves of a workgroup load
// the same 64 operand rows four times over (16 quads each) in four dependent trips; here a lane keeps its row's 16 accumulators,
// every operand quad is loaded ONCE and all of them are in flight together.  W rows come through scalar loads (uniform
// addresses).  The same chain of fused multiply-adds per output element (k ascending): bit-identical to k_gemm_skinny.
// Epilogue as k_gemm_skinny<64>: ReLU / ReLU-backward mask, the second product post_out = [act(out) | 1 0 0 0] @ post_W.
static constexpr int QT_ROW16_INF = 8;
__global__ __launch_bounds__(64) void k_gemm_row16(GemmArgs g) {
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    const int t = threadIdx.x;
    const int64_t rows = qt_rows(g.n_dev, g.M);
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    if (row0 >= rows) return;
    const int nquad = g.K >> 2;
    build_quad_table(g.A, qptr, qstr, nquad);          // (nquad <= 64 = the threads of this workgroup: one entry each)
    __syncthreads();
    const int64_t row = row0 + t;
    const bool ok = row < rows;
    float4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto step = [&](float a, int k) {
        const float* __restrict__ wr = g.B + (int64_t)k * 16;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 w = *reinterpret_cast<const float4*>(wr + 4 * c);
            acc[c].x = fmaf(a, w.x, acc[c].x); acc[c].y = fmaf(a, w.y, acc[c].y);
            acc[c].z = fmaf(a, w.z, acc[c].z); acc[c].w = fmaf(a, w.w, acc[c].w);
        }
    };
    constexpr int INF = QT_ROW16_INF;                    // operand quads in flight per trip
    for (int Q = 0; Q < nquad; Q += INF) {
        float4 aq[INF];
#pragma unroll
        for (int u = 0; u < INF; ++u) {
            aq[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && Q + u < nquad) aq[u] = gload4(qptr[Q + u] + row * qstr[Q + u]);
        }
#pragma unroll
        for (int u = 0; u < INF; ++u)
            if (Q + u < nquad) {
                step(aq[u].x, 4 * (Q + u)); step(aq[u].y, 4 * (Q + u) + 1); step(aq[u].z, 4 * (Q + u) + 2); step(aq[u].w, 4 * (Q + u) + 3);
            }
    }
    if (!ok) return;
    if (g.act == QT_ACT_RELU) {
        const float d = g.drop ? g.drop[row] : 1.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = act_quad(acc[c], QT_ACT_RELU, d, 0.0f);
    }
    if (g.act == QT_ACT_RELU_BWD) {
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = relu_bwd_quad(acc[c], *reinterpret_cast<const float4*>(g.res + row * g.res_stride + 4 * c));
    }
    if (g.post_W) *reinterpret_cast<float4*>(g.post_out + row * 4) = post_product(acc, g.post_W);
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<float4*>(g.out + row * 16 + 4 * c) = acc[c];
}

// ---- the decoder head's backward products in ONE launch, one lane per node row:
//   G = relu'(Y) (.) (gU @ Wb2)          (N, 16): the gradient at fc_out1's output (Wb2 (4, 16) = the coefficient columns of
//                                         fc_out2 transposed); stored -- the deferred weight gradient of fc_out1 reads it
//   planes = G @ Wb1^T                   (K, N, Ca | Cbb): the data gradient of fc_out1, Wb1 (K (Ca + Cbb), 16) = its rows
// Replaces a k_gemm_skinny launch (gU -> G) and a k_gemm_fwd<2, 128> launch (G -> planes: 16 x 60 on the MFMA) whose operand G made
// a round trip through memory in between: 25 -> ~11 us per decoder step.  The chains are the k-ordered fused multiply-adds of the
// two launches (v_mfma_f32_32x32x2_f32 accumulates in k order): bit-identical planes.
struct HeadDgradArgs {
    const float *gU, *Wb2, *Y, *Wb1;
    float *G, *out, *outb;
    int N, K, Cb, Cbb, out_sm;
    const int32_t* n_dev;
};
__global__ __launch_bounds__(64) void k_head_dgrad(HeadDgradArgs g) {
    const int64_t rows = qt_rows(g.n_dev, g.N);
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if ((int64_t)blockIdx.x * 64 >= rows) return;
    const bool ok = row < rows;
    const int64_t r = ok ? row : rows - 1;              // (clamped loads, predicated stores)
    const float4 gu = gload4(g.gU + r * 4);
    float4 y[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) y[c] = gload4(g.Y + r * 16 + 4 * c);
    float G[16];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        const float guv[4] = {gu.x, gu.y, gu.z, gu.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 w = *reinterpret_cast<const float4*>(g.Wb2 + k * 16 + 4 * c);
            a.x = fmaf(guv[k], w.x, a.x); a.y = fmaf(guv[k], w.y, a.y); a.z = fmaf(guv[k], w.z, a.z); a.w = fmaf(guv[k], w.w, a.w);
        }
        a = relu_bwd_quad(a, y[c]);
        G[4 * c] = a.x; G[4 * c + 1] = a.y; G[4 * c + 2] = a.z; G[4 * c + 3] = a.w;
        if (ok) *reinterpret_cast<float4*>(g.G + row * 16 + 4 * c) = a;
    }
    const int ct = g.Cb + g.Cbb;
    for (int pl = 0; pl < g.K; ++pl) {
        for (int ch = 0; ch < ct; ch += 4) {
            const float* __restrict__ wr = g.Wb1 + (int64_t)(pl * ct + ch) * 16;      // rows of the four output columns (uniform)
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // the reduction order of k_gemm_fwd's MFMA stream (v_mfma_f32_32x32x2_f32: lanes 0-31 carry k = 8 j + i, lanes 32-63
                // k = 8 j + 4 + i of instruction i): 0 4 1 5 2 6 3 7 | 8 12 9 13 10 14 11 15 -- bit-identical planes
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float4 wl = *reinterpret_cast<const float4*>(wr + q * 16 + 8 * j);
                    const float4 wh = *reinterpret_cast<const float4*>(wr + q * 16 + 8 * j + 4);
                    a = fmaf(G[8 * j + 0], wl.x, a); a = fmaf(G[8 * j + 4], wh.x, a);
                    a = fmaf(G[8 * j + 1], wl.y, a); a = fmaf(G[8 * j + 5], wh.y, a);
                    a = fmaf(G[8 * j + 2], wl.z, a); a = fmaf(G[8 * j + 6], wh.z, a);
                    a = fmaf(G[8 * j + 3], wl.w, a); a = fmaf(G[8 * j + 7], wh.w, a);
                }
                o[q] = a;
            }
            if (!ok) continue;
            const float4 v = make_float4(o[0], o[1], o[2], o[3]);
            if (ch < g.Cb)
                *reinterpret_cast<float4*>(plane_piece(g.out, pl, row, ch, g.Cb, g.N, g.out_sm, g.Cb)) = v;
            else
                *reinterpret_cast<float4*>(plane_piece(g.outb, pl, row, ch - g.Cb, g.Cbb, g.N, g.out_sm, g.Cbb)) = v;
        }
    }
}

// ---- bf16x3 variant of the forward / data-gradient GEMM -------------------------------------------------------------
// fp32 MFMA runs at the VALU FLOP rate on gfx950 and bounds k_gemm_fwd (HISTORY.md section C).  Here every fp32 operand
// is split into three bf16 terms (x = hi + mid + lo, each rounded to nearest) and a product group is six bf16 MFMAs
// (hi.hi, hi.mid, mid.hi, hi.lo, lo.hi, mid.mid) accumulated in fp32: the dropped terms are O(2^-24) of the product,
// i.e. fp32-level error, at 16 k per 32-cycle instruction instead of 2 k per 64-cycle instruction.

__device__ __forceinline__ void split3(float x, __bf16* h, __bf16* m, __bf16* l) {
    const __bf16 hh = (__bf16)x;
    const float r = x - (float)hh;
    const __bf16 mm = (__bf16)r;
    const float r2 = r - (float)mm;
    *h = hh; *m = mm; *l = (__bf16)r2;
}

template <int NT, int KWT>
__global__ __launch_bounds__(256) void k_gemm_fwd3(GemmArgs g) {
    constexpr int BNT = 32 * NT;
    constexpr int PITCH = KWT + 8;          // bf16 elements; row pitch in bytes = 16 (mod 32): conflict-free ds_read_b128
    constexpr int PLANE = BNT * PITCH;      // one of the three split planes of W^T: Bt[x][column][k]
    static_assert(3 * PLANE * 2 >= BM * 64 * 4, "LDS staging tile does not fit in the W buffer");
    __shared__ __attribute__((aligned(16))) __bf16 Bt[3 * PLANE];
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int j0 = blockIdx.y * BNT;
    const int64_t rows = qt_rows(g.n_dev, g.M);
    if (i0 >= rows) return;
    const int nquad = g.K >> 2;
    build_quad_table(g.A, qptr, qstr, nquad);
    const int64_t my_row = i0 + wave * 32 + l32;
    const bool row_ok = my_row < rows;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    for (int k0 = 0; k0 < g.K; k0 += KWT) {
        const int kn = min(KWT, g.K - k0);           // multiple of 4
        const int kn16 = (kn + 15) & ~15;
        __syncthreads();
        // W chunk -> LDS, transposed and split: pairs of k rows so that every LDS store is a packed 32-bit word
        for (int e = t; e < (kn16 / 2) * (BNT / 4); e += 256) {
            const int kp = e / (BNT / 4), jq = (e % (BNT / 4)) * 4;
            float w[2][4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kb = 2 * kp + u;
                float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kb < kn && j0 + jq < g.NB) f = *reinterpret_cast<const float4*>(g.B + (int64_t)(k0 + kb) * g.NB + j0 + jq);
                w[u][0] = f.x; w[u][1] = f.y; w[u][2] = f.z; w[u][3] = f.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                __bf16 h0, m0, l0, h1, m1, l1;
                split3(w[0][c], &h0, &m0, &l0);
                split3(w[1][c], &h1, &m1, &l1);
                typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
                const int o = (jq + c) * PITCH + 2 * kp;
                *reinterpret_cast<bf16x2*>(&Bt[o]) = bf16x2{h0, h1};
                *reinterpret_cast<bf16x2*>(&Bt[PLANE + o]) = bf16x2{m0, m1};
                *reinterpret_cast<bf16x2*>(&Bt[2 * PLANE + o]) = bf16x2{l0, l1};
            }
        }
        __syncthreads();
        // MFMA stream: step J covers k = 16 J .. 16 J + 15; this lane feeds k = 16 J + 8 half .. + 7 (two quads of its row)
        const int q0 = k0 >> 2, qn = kn >> 2, nJ = kn16 >> 4;
        auto ldq = [&](int q) {
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row_ok && q < qn) r = gload4(qptr[q0 + q] + my_row * qstr[q0 + q]);
            return r;
        };
        float4 c0 = ldq(2 * half), c1 = ldq(2 * half + 1);                 // J = 0
        float4 n0 = ldq(4 + 2 * half), n1 = ldq(4 + 2 * half + 1);         // J = 1
        for (int J = 0; J < nJ; ++J) {
            const float av[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            c0 = n0; c1 = n1;
            n0 = ldq(4 * (J + 2) + 2 * half);
            n1 = ldq(4 * (J + 2) + 2 * half + 1);
            bf16x8 ah, am, al;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __bf16 h, m, l;
                split3(av[i], &h, &m, &l);
                ah[i] = h; am[i] = m; al[i] = l;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int o = (nt * 32 + l32) * PITCH + 16 * J + 8 * half;
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&Bt[o]);
                const bf16x8 bm = *reinterpret_cast<const bf16x8*>(&Bt[PLANE + o]);
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&Bt[2 * PLANE + o]);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[nt], 0, 0, 0);     // small terms first
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[nt], 0, 0, 0);
            }
        }
    }
    stage_and_store<NT>(acc, reinterpret_cast<float*>(Bt), g, i0, j0, rows);
}

// Data-gradient GEMM as a split-bf16 product (gradients only): out planes = A (N x K fp32 rows) @ B, with B^T given as two bf16
// terms per element (Bhi + Blo ~ B, qt_split_bf16) and A split on the fly; three bf16 MFMAs per product group (lo.hi, hi.lo, hi.hi:
// the dropped lo.lo term is 2^-16 of the product) at 16 k per 32-cycle instruction.  The fp32-MFMA form of this product runs at
// 60 % of the fp32-MFMA peak for hidden 32 (K = 128): the matrix pipe, not memory, sets its time.
template <int NT>
__global__ __launch_bounds__(256, 4) void k_gemm_sb(GemmArgs g, const __bf16* __restrict__ Bhi, const __bf16* __restrict__ Blo) {
    constexpr int KWT = 64, BNT = 32 * NT;
    constexpr int PITCH = KWT + 8;          // bf16 elements; row pitch in bytes = 16 (mod 32): conflict-free ds_read_b128
    constexpr int PLANE = BNT * PITCH;
    constexpr int LDS_BYTES = 2 * PLANE * 2 > BM * 64 * 4 ? 2 * PLANE * 2 : BM * 64 * 4;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    __bf16* Bt = reinterpret_cast<__bf16*>(lds);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * BM;
    const int j0 = blockIdx.y * BNT;
    const int64_t rows = qt_rows(g.n_dev, g.M);
    if (i0 >= rows) return;
    const int64_t my_row = i0 + wave * 32 + l32;
    const bool row_ok = my_row < rows;
    const float* arow = g.A.a0 + my_row * g.A.lda0;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    for (int k0 = 0; k0 < g.K; k0 += KWT) {
        const int kn = min(KWT, g.K - k0);           // multiple of 16 (checked by the host entry)
        __syncthreads();
        const int k8 = kn >> 3;
        for (int e = t; e < BNT * k8; e += 256) {     // both bf16 planes of the weight chunk: straight 16-byte copies
            const int c = e / k8, kq = e - c * k8;
            u32x4 wh = {0u, 0u, 0u, 0u}, wl = wh;
            if (j0 + c < g.NB) {
                const int64_t o = (int64_t)(j0 + c) * g.K + k0 + 8 * kq;
                wh = *reinterpret_cast<const u32x4*>(Bhi + o);
                wl = *reinterpret_cast<const u32x4*>(Blo + o);
            }
            *reinterpret_cast<u32x4*>(&Bt[c * PITCH + 8 * kq]) = wh;
            *reinterpret_cast<u32x4*>(&Bt[PLANE + c * PITCH + 8 * kq]) = wl;
        }
        __syncthreads();
        const int nJ = kn >> 4;
        auto ldk = [&](int J, int u) {              // quad u of this lane's eight k of step J
            float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row_ok && J < nJ) r = gload4(arow + k0 + 16 * J + 8 * half + 4 * u);
            return r;
        };
        float4 c0 = ldk(0, 0), c1 = ldk(0, 1), n0 = ldk(1, 0), n1 = ldk(1, 1);
        for (int J = 0; J < nJ; ++J) {
            const float av[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
            c0 = n0; c1 = n1;
            n0 = ldk(J + 2, 0);
            n1 = ldk(J + 2, 1);
            bf16x8 ah, al;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const __bf16 h = (__bf16)av[i];
                ah[i] = h;
                al[i] = (__bf16)(av[i] - (float)h);
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int o = (nt * 32 + l32) * PITCH + 16 * J + 8 * half;
                const bf16x8 bh = *reinterpret_cast<const bf16x8*>(&Bt[o]);
                const bf16x8 bl = *reinterpret_cast<const bf16x8*>(&Bt[PLANE + o]);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[nt], 0, 0, 0);     // small terms first
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[nt], 0, 0, 0);
                acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[nt], 0, 0, 0);
            }
        }
    }
    stage_and_store<NT>(acc, reinterpret_cast<float*>(lds), g, i0, j0, rows);      // (g.act == QT_ACT_NONE: no activation)
}

constexpr int WR = 32;
// FW feature waves x (4 / FW) row groups, CT column tiles of 32.  The MFMA count per pass is what bounds this kernel, so
// a narrow weight must not pay for the full 128 x 64 tile: with FW < 4 the spare waves take a share of every pass's rows
// (their partial tiles are added through LDS at the end, in a fixed order), with CT = 1 the second column tile is skipped.
template <int FW, int CT>
__device__ __forceinline__ void wgrad_body(const PlaneSrc& A, const float* __restrict__ G, int M, int NB, int64_t rbeg,
                                           int64_t rend, float* obase, int accumulate, int jt, int ldg, int gpl = 0,
                                           int64_t gps = 0) {       // gpl > 0: G columns in planes of gpl floats, gps apart
    constexpr int RG = 4 / FW;             // row groups
    constexpr int KS = WR / 2 / RG;        // k-steps (2 rows each) per row group and pass
    constexpr int BMF = FW * 32;           // features per block
    // A tiles hold only the BMF features this block owns (narrow weights then fit 4 workgroups per CU); the same floats
    // later park the row groups' partial tiles
    constexpr int RED_FLOATS = (RG - 1) * FW * CT * 16 * 64;
    constexpr int AS_FLOATS = 2 * WR * BMF > RED_FLOATS ? 2 * WR * BMF : RED_FLOATS;
    __shared__ __attribute__((aligned(16))) float As_pool[AS_FLOATS];
    auto As = [&](int buf, int row, int col) -> float& { return As_pool[(buf * WR + row) * BMF + col]; };
    __shared__ __attribute__((aligned(16))) float Gs[2][WR][BN];
    __shared__ const float* qptr[MAXQ];
    __shared__ int qstr[MAXQ];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l32 = lane & 31, half = lane >> 5;
    const int fw = wave % FW, rg = wave / FW;
    const int f0 = blockIdx.x * BMF, j0 = jt * BN;
    const int nquad = M >> 2;
    build_quad_table(A, qptr, qstr, nquad);
    __syncthreads();
    // staging roles: A tile = 32 rows x 32 quads -> 4 float4 per thread; G tile = 32 rows x 16 quads -> 2 per thread.
    // Within one load instruction the 8 threads of a row take 8 CONSECUTIVE quads (128 contiguous bytes where the quads
    // share a plane part); giving each thread 4 consecutive quads instead made every 4-lane group of the texture addresser
    // span four 64-byte segments.
    const int a_row = t >> 3, a_q = t & 7;
    const int g_row = t >> 3, g_q = t & 7;
    // two passes of operands in flight: the rows of this kernel come from HBM (activations saved by the forward pass),
    // and with one pass of prefetch every group of weights ran at ~3 TB/s whatever its MFMA load
    float4 pa[2][4], pg[2][2];
    auto fetch = [&](int64_t r0, float4 (&qa)[4], float4 (&qg)[2]) {
        const int64_t ra = r0 + a_row;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ql = u * 8 + a_q;
            const int Q = (f0 >> 2) + ql;
            qa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ra < rend && Q < nquad && ql < BMF / 4) qa[u] = gload4(qptr[Q] + ra * qstr[Q]);
        }
        const int64_t rgw = r0 + g_row;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int jq = (u * 8 + g_q) * 4;
            qg[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rgw < rend && j0 + jq < NB && jq < CT * 32) {
                const int j = j0 + jq, pl = gpl ? j / gpl : 0;
                qg[u] = gload4(G + pl * gps + rgw * ldg + (j - pl * gpl));
            }
        }
    };
    auto stash = [&](int buf, const float4 (&qa)[4], const float4 (&qg)[2]) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if ((u * 8 + a_q) * 4 < BMF) *reinterpret_cast<float4*>(&As(buf, a_row, (u * 8 + a_q) * 4)) = qa[u];
#pragma unroll
        for (int u = 0; u < 2; ++u) *reinterpret_cast<float4*>(&Gs[buf][g_row][(u * 8 + g_q) * 4]) = qg[u];
    };
    f32x16 acc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
    auto mfma_pass = [&](int buf) {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const int ks = rg * KS + k;
            const float a = As(buf, 2 * ks + half, fw * 32 + l32);
#pragma unroll
            for (int c = 0; c < CT; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Gs[buf][2 * ks + half][c * 32 + l32], acc[c], 0, 0, 0);
        }
    };
    if (rbeg < rend) {
        // LDS buffer b holds pass p (p even: b = 0), register set (p + 1) & 1 holds pass p + 1, set p & 1 is loaded with
        // pass p + 2 while pass p is multiplied; rows past `rend` load as zeros, so the tail needs no special case
        fetch(rbeg, pa[0], pg[0]);
        fetch(rbeg + WR, pa[1], pg[1]);
        stash(0, pa[0], pg[0]);
        __syncthreads();
        for (int64_t r0 = rbeg; r0 < rend; r0 += 2 * WR) {
            fetch(r0 + 2 * WR, pa[0], pg[0]);
            mfma_pass(0);
            stash(1, pa[1], pg[1]);
            __syncthreads();
            fetch(r0 + 3 * WR, pa[1], pg[1]);
            mfma_pass(1);                        // an all-zero pass when r0 + WR >= rend
            stash(0, pa[0], pg[0]);
            __syncthreads();
        }
    }
    if constexpr (RG > 1) {
        // add the row groups' partial tiles: groups 1.. park theirs in LDS (the A buffers are free), group 0 adds in order
        float* red = As_pool;
        if (rg > 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((((rg - 1) * FW + fw) * CT + c) * 16 + r) * 64 + lane] = acc[c][r];
        }
        __syncthreads();
        if (rg > 0) return;
#pragma unroll
        for (int g2 = 1; g2 < RG; ++g2)
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][r] += red[((((g2 - 1) * FW + fw) * CT + c) * 16 + r) * 64 + lane];
    }
#pragma unroll
    for (int jt = 0; jt < CT; ++jt) {
        const int j = j0 + jt * 32 + l32;
        if (j >= NB) continue;
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {      // all slab reads first: 16 independent loads in flight
            const int i = f0 + fw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            old[r] = (accumulate && i < M) ? obase[(int64_t)i * NB + j] : 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = f0 + fw * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (i < M) obase[(int64_t)i * NB + j] = old[r] + acc[jt][r];
        }
    }
}

// MODE 1: part[blockIdx.z] = A[rows]^T @ G[rows] over this block's row chunk.  Block = 32 FW features x 32 CT
// columns of the weight gradient; the reduction runs over node rows in passes of 32 rows: float4 global loads ->
// registers (prefetch of the next pass) -> double-buffered LDS.
template <int FW, int CT>
__global__ __launch_bounds__(256) void k_gemm_wgrad(GemmArgs g) {
    const int64_t rbeg = (int64_t)blockIdx.z * g.row0_step;
    const int64_t rend = min((int64_t)qt_rows(g.n_dev, g.A.N), rbeg + g.row0_step);
    wgrad_body<FW, CT>(g.A, g.B, g.M, g.NB, rbeg, rend, g.out + (int64_t)blockIdx.z * g.M * g.NB, g.accumulate, blockIdx.y, g.NB);
}

// The same reduction for up to 16 uses of ONE weight in a single launch (the rollout steps of a pass): z-blocks
// [zend[s-1], zend[s]) walk the node rows of use s; every z-block owns its slab, qt_colsum adds them in fixed order.
constexpr int MAXSEG = 16;
struct WgradGroup {
    const float* a0[MAXSEG];
    const float* a_rest[MAXSEG];
    const float* a0b[MAXSEG];
    const float* a_restb[MAXSEG];
    const float* S[MAXSEG];
    const float* G[MAXSEG];
    const int32_t* n_dev[MAXSEG];
    int N[MAXSEG], zend[MAXSEG], lda0[MAXSEG], lda0b[MAXSEG];
    int nseg, Ka, Ca, Cab, Ks, Co, rows, sm;
    float* part;
    // Gn weights per use (the stacks of one layer, qt_proj_group): grid y = (group, column tile); group g reads plane 0 at
    // a0 + g gsA and the gradient rows at G + g gsG (row stride ldg), and owns slab (z, g) of part
    int Gn, ytiles, ldg, gpl, per_node;      // per_node: gsA / gsG are floats per node of the use (x N[s])
    int64_t gsA, gsG;
};
template <int FW, int CT>
__global__ __launch_bounds__(256) void k_gemm_wgrad_group(WgradGroup w) {
    int s = 0;
    while (s + 1 < w.nseg && (int)blockIdx.z >= w.zend[s]) ++s;
    const int zl = blockIdx.z - (s ? w.zend[s - 1] : 0);
    PlaneSrc A;
    A.a0 = w.a0[s]; A.a_rest = w.a_rest[s]; A.a0b = w.a0b[s]; A.a_restb = w.a_restb[s]; A.S = w.S[s];
    A.Ka = w.Ka; A.Ca = w.Ca; A.Cab = w.Cab; A.Ks = w.Ks; A.N = w.N[s]; A.lda0 = w.lda0[s]; A.lda0b = w.lda0b[s]; A.sm = w.sm;
    const int M = w.Ka * (w.Ca + w.Cab) + w.Ks;
    const int64_t rbeg = (int64_t)zl * w.rows;
    const int64_t rend = min((int64_t)qt_rows(w.n_dev[s], w.N[s]), rbeg + w.rows);
    const int grp = blockIdx.y / w.ytiles, jt = blockIdx.y - grp * w.ytiles;
    const int64_t gmul = w.per_node ? (int64_t)grp * w.N[s] : grp;
    A.a0 += gmul * w.gsA;
    wgrad_body<FW, CT>(A, w.G[s] + gmul * w.gsG, M, w.Co, rbeg, rend, w.part + ((int64_t)blockIdx.z * w.Gn + grp) * M * w.Co, 0, jt, w.ldg, w.gpl,
                       (int64_t)w.N[s] * w.gpl);
}

// 32 columns x 32 row groups per workgroup, four slabs in flight per thread; fixed summation order (deterministic).
// (With 8 row groups and one load in flight the 640 slabs of a grouped weight gradient took 30 us: a latency chain.)
__global__ __launch_bounds__(1024) void k_colsum(const float* __restrict__ part, int nblk, int64_t len, float* __restrict__ out) {
    __shared__ float sm[32][33];
    const int cl = threadIdx.x & 31, r = threadIdx.x >> 5;
    const int64_t c = (int64_t)blockIdx.x * 32 + cl;
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    if (c < len) {
        int i = r;
        for (; i + 96 < nblk; i += 128) {
            a0 += part[(int64_t)i * len + c];
            a1 += part[(int64_t)(i + 32) * len + c];
            a2 += part[(int64_t)(i + 64) * len + c];
            a3 += part[(int64_t)(i + 96) * len + c];
        }
        for (; i < nblk; i += 32) a0 += part[(int64_t)i * len + c];
    }
    sm[r][cl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (r == 0 && c < len) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 32; ++k) s += sm[k][cl];
        out[c] = s;
    }
}

// tile variant by weight shape: feature waves 1 / 2 / 4 for up to 32 / 64 / more features, one column tile up to 32 columns
inline int wgrad_fw(int M) { return M <= 32 ? 1 : (M <= 64 ? 2 : 4); }
#define QT_WGRAD_DISPATCH(K, M_, Co_, grid_, stream_, arg_)                                                         \
    do {                                                                                                            \
        const int fw_ = wgrad_fw(M_);                                                                               \
        const bool one_ = (Co_) <= 32;                                                                              \
        if (fw_ == 1 && one_) hipLaunchKernelGGL((K<1, 1>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_);     \
        else if (fw_ == 1) hipLaunchKernelGGL((K<1, 2>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_);        \
        else if (fw_ == 2 && one_) hipLaunchKernelGGL((K<2, 1>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_); \
        else if (fw_ == 2) hipLaunchKernelGGL((K<2, 2>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_);        \
        else if (one_) hipLaunchKernelGGL((K<4, 1>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_);            \
        else hipLaunchKernelGGL((K<4, 2>), grid_, dim3(256), 0, (hipStream_t)(stream_), arg_);                      \
    } while (0)
// node rows per z-block of the weight-gradient launches, single and grouped
constexpr int WGRAD_ROWS = 512;      // 11.02 ms per training step against 11.07 (1024) and 11.20 (256)

}  // namespace

// Tile width of a plain product by its output width: the fewest 32-column MFMA tiles over all column blocks (NB = 280: 3 blocks of
// 3 tiles = 9 tiles instead of 3 x 4 = 12), ties to the wider block (A is re-read per block).
static inline int gemm_nt(int NB) {
    int best = 4, cost = qt_cdiv(NB, 128) * 4;
    for (int nt = 3; nt >= 2; --nt) {
        const int c = qt_cdiv(NB, 32 * nt) * nt;
        if (c < cost) {
            best = nt;
            cost = c;
        }
    }
    return NB <= 64 ? 2 : best;
}
static constexpr int QT_GEMM_KWT3 = 128;
static constexpr int QT_GEMM_KWT4 = 64;      // k rows of W staged per pass by the 128-column tiles (NT = 4)
static void launch_gemm_fwd(const GemmArgs& g, int N, int G, hipStream_t stream) {
    switch (gemm_nt(g.NB)) {
        case 2: hipLaunchKernelGGL((k_gemm_fwd<2, 128>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 64), G), dim3(256), 0, stream, g); break;
        case 3: hipLaunchKernelGGL((k_gemm_fwd<3, QT_GEMM_KWT3>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 96), G), dim3(256), 0, stream, g); break;
        default: hipLaunchKernelGGL((k_gemm_fwd<4, QT_GEMM_KWT4>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 128), G), dim3(256), 0, stream, g); break;
    }
}

// (declared in qt_gemm.h) one 128-row tile per workgroup, all 4h gate columns in its 32 NT columns
void gemm_fwd_cell_launch(const void* gemm_args, int N, hipStream_t stream) {
    const GemmArgs& g = *static_cast<const GemmArgs*>(gemm_args);
    const dim3 grid(qt_cdiv(N, BM), 1, 1);
    if (g.h == 32)
        hipLaunchKernelGGL((k_gemm_fwd<4, QT_GEMM_KWT4, 8>), grid, dim3(256), 0, stream, g);
    else if (g.h == 16)
        hipLaunchKernelGGL((k_gemm_fwd<2, 128, 4>), grid, dim3(256), 0, stream, g);
    else
        hipLaunchKernelGGL((k_gemm_fwd<2, 128, 2>), grid, dim3(256), 0, stream, g);
}

extern "C" int qt_dense2(const float* a0, int lda0, const float* a_rest, const float* a0b, int lda0b, const float* a_restb, int Ka,
                         int Ca, int Cab,
                         const float* W, const float* WT, const float* S, int Ks, const float* Ws, int Kb, int Cb, int Cbb, int N,
                         const int32_t* n_dev, int act, const float* res, int res_stride, const float* drop, float* out,
                         float* outb, int planes_sm, const float* post_W, float* post_out, void* stream) {
    QT_ARG((W || WT) && out && Kb >= 1 && Cb >= 1 && Cbb >= 0 && (Cbb == 0 || outb), "bad arguments");
    QT_ARG((post_W == nullptr) == (post_out == nullptr) && (!post_W || (W && Kb * (Cb + Cbb) == 16 && (((uintptr_t)post_W | (uintptr_t)post_out) & 15) == 0)),
           "the second product needs 16 output columns, W (not WT) and 16-byte aligned post_W (20, 4) / post_out (N, 4)");
    QT_ARG(act != QT_ACT_RELU_BWD || (res && res_stride >= Kb * (Cb + Cbb) && res_stride % 4 == 0 && W && Kb * (Cb + Cbb) <= 16 && Kb * (Cb + Cbb) > 4),
           "QT_ACT_RELU_BWD: res = the forward output (N, res_stride), 8 .. 16 output columns, W (not WT)");
    QT_ARG((Ks == 0) || Ws || WT, "Ws missing");
    QT_ARG(Ks == 0 || WT || Ws == W + (int64_t)Ka * (Ca + Cab) * Kb * (Cb + Cbb), "Ws must follow W contiguously ([W ; Ws] is one matrix)");
    QT_ARG(act == QT_ACT_NONE || (Kb == 1 && Cbb == 0), "activation needs one undivided output plane");
    QT_ARG(Cb % 4 == 0 && Cbb % 4 == 0, "Cb and Cbb must be multiples of 4 (float4 stores)");
    QT_ARG((((uintptr_t)W | (uintptr_t)WT) & 15) == 0, "W / WT must be 16-byte aligned");
    QT_ARG(act != QT_ACT_TANH_RES || res, "QT_ACT_TANH_RES needs res");
    GemmArgs g = {};
    if (int rc = plane_src(&g.A, __func__, a0, lda0, a_rest, a0b, lda0b, a_restb, Ka, Ca, Cab, S, Ks, N, planes_sm & 1)) return rc;
    g.out_sm = (planes_sm >> 1) & 1;
    if (N <= 0) return QT_OK;
    g.B = W; g.BT = WT; g.M = N; g.K = Ka * (Ca + Cab) + Ks; g.NB = Kb * (Cb + Cbb);
    g.outb = outb; g.Cbb = Cbb;
    g.Kb = Kb; g.Cb = Cb; g.act = act; g.res = res; g.res_stride = res_stride; g.drop = drop; g.out = out; g.n_dev = n_dev;
    g.post_W = post_W; g.post_out = post_out;
    // default: exact fp32 MFMA (bit-for-bit a k-ordered fmaf chain).  QT_GEMM_BF16X3=1 opts into the bf16x3 split
    // kernels (fp32-level error, ~8 % faster on these memory/latency-shaped GEMMs: measured 27.7 vs 30.1 us).
    static const bool exact_fp32 = getenv("QT_GEMM_BF16X3") == nullptr;
    if (g.NB <= 16 && W) {       // (wide outputs of short reductions measured slower here: 24.5 vs 14.5 us)
        static const bool no_row16 = getenv("QT_GEMM_NO_ROW16") != nullptr;       // (A/B switch)
        if (g.NB <= 4)
            hipLaunchKernelGGL((k_gemm_skinny<256>), dim3(qt_cdiv(N, 256), 1, 1), dim3(256), 0, (hipStream_t)stream, g);
        else if (!no_row16 && g.NB == 16 && Kb == 1 && Cbb == 0 && act != QT_ACT_TANH_RES && g.K <= 256)
            hipLaunchKernelGGL(k_gemm_row16, dim3(qt_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, g);
        else
            hipLaunchKernelGGL((k_gemm_skinny<64>), dim3(qt_cdiv(N, 64), qt_cdiv(g.NB, 16), 1), dim3(256), 0, (hipStream_t)stream, g);
    } else if (exact_fp32) {
        launch_gemm_fwd(g, N, 1, (hipStream_t)stream);
    } else {
        if (g.NB > 64)
            hipLaunchKernelGGL((k_gemm_fwd3<4, 64>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 128), 1), dim3(256), 0, (hipStream_t)stream, g);
        else
            hipLaunchKernelGGL((k_gemm_fwd3<2, 128>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 64), 1), dim3(256), 0, (hipStream_t)stream, g);
    }
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_head_dgrad(const float* gU, const float* Wb2, const float* Y, const float* Wb1, int K, int Cb, int Cbb, int N,
                             const int32_t* n_dev, float* G, float* out, float* outb, int out_sm, void* stream) {
    QT_ARG(gU && Wb2 && Y && Wb1 && G && out && K >= 1 && Cb > 0 && Cb % 4 == 0 && Cbb >= 0 && Cbb % 4 == 0 && (Cbb == 0 || outb), "bad arguments");
    QT_ARG((((uintptr_t)gU | (uintptr_t)Wb2 | (uintptr_t)Y | (uintptr_t)Wb1 | (uintptr_t)G | (uintptr_t)out | (uintptr_t)outb) & 15) == 0,
           "operands must be 16-byte aligned");
    if (N <= 0) return QT_OK;
    HeadDgradArgs g = {gU, Wb2, Y, Wb1, G, out, outb, N, K, Cb, Cbb, out_sm != 0, n_dev};
    hipLaunchKernelGGL(k_head_dgrad, dim3(qt_cdiv(N, 64)), dim3(64), 0, (hipStream_t)stream, g);
    QT_LAUNCHED();
    return QT_OK;
}

// G independent products in one launch (grid z = group): group g multiplies [A_g | S], A_g = Ka planes (N, Ca) starting at
// A + g gsA, with W_g and writes Kb planes (N, Cb) starting at out + g gsO (row stride ldo).
// The eight GraphConv stacks of a GConvLSTM with attention convolutions (model/model.py:394-424) run layer by layer: group g
// is stack g's projection [q | k | v | skip], read from and written to blocks of arrays shared by all stacks.
extern "C" int qt_proj_group(const float* A, int lda, int64_t gsA, int Ka, int Ca, const float* S, const float* W, const float* WT,
                             int64_t gsW, int G, int Kb, int Cb, float* out, int ldo, int64_t gsO, int reverse, int N,
                             const int32_t* n_dev, void* stream) {
    QT_ARG((W || WT) && out && G >= 1 && G <= 65535 && Kb >= 1 && Cb >= 4 && Cb % 4 == 0 && Ka >= 1, "bad arguments");
    if (ldo == 0) ldo = Cb;
    QT_ARG(ldo >= Cb && ldo % 4 == 0 && gsA % 4 == 0 && gsW % 4 == 0 && gsO % 4 == 0, "strides must be multiples of 4 floats");
    QT_ARG(Ka == 1 || lda == 0 || lda == Ca, "several input planes must be dense");
    QT_ARG((((uintptr_t)W | (uintptr_t)WT | (uintptr_t)out) & 15) == 0, "W / WT / out must be 16-byte aligned");
    GemmArgs g = {};
    if (int rc = plane_src(&g.A, __func__, A, lda, Ka > 1 ? A + (int64_t)N * Ca : nullptr, nullptr, 0, nullptr, Ka, Ca, 0, S, S ? 4 : 0, N))
        return rc;
    if (N <= 0) return QT_OK;
    g.B = W; g.BT = WT; g.M = N; g.K = Ka * Ca + (S ? 4 : 0); g.NB = Kb * Cb;
    g.Kb = Kb; g.Cb = Cb; g.out = out; g.n_dev = n_dev;
    g.ldo = ldo; g.gsA = gsA; g.gsB = gsW; g.gsO = gsO;
    g.zrev = reverse != 0;
    launch_gemm_fwd(g, N, G, (hipStream_t)stream);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_dense_sb(const float* A, int lda, int K, const void* Whi, const void* Wlo, int Kb, int Cb, int Cbb, int N,
                           const int32_t* n_dev, float* out, float* outb, void* stream) {
    QT_ARG(A && Whi && Wlo && out && Kb >= 1 && Cb >= 4 && Cb % 4 == 0 && Cbb >= 0 && Cbb % 4 == 0 && (Cbb == 0 || outb), "bad arguments");
    if (lda == 0) lda = K;
    QT_ARG(K >= 16 && K % 16 == 0 && lda >= K && lda % 4 == 0, "the reduction length must be a multiple of 16");
    QT_ARG((((uintptr_t)A | (uintptr_t)Whi | (uintptr_t)Wlo | (uintptr_t)out | (uintptr_t)outb) & 15) == 0, "operands must be 16-byte aligned");
    if (N <= 0) return QT_OK;
    GemmArgs g = {};
    g.A.a0 = A; g.A.lda0 = lda; g.A.N = N; g.A.Ka = 1; g.A.Ca = K;
    g.M = N; g.K = K; g.NB = Kb * (Cb + Cbb); g.Kb = Kb; g.Cb = Cb; g.Cbb = Cbb; g.out = out; g.outb = outb; g.n_dev = n_dev;
    if (g.NB > 64)
        hipLaunchKernelGGL((k_gemm_sb<4>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 128)), dim3(256), 0, (hipStream_t)stream, g, (const __bf16*)Whi,
                           (const __bf16*)Wlo);
    else
        hipLaunchKernelGGL((k_gemm_sb<2>), dim3(qt_cdiv(N, BM), qt_cdiv(g.NB, 64)), dim3(256), 0, (hipStream_t)stream, g, (const __bf16*)Whi,
                           (const __bf16*)Wlo);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_dense(const float* a0, const float* a_rest, int Ka, int Ca, const float* W, const float* S, int Ks,
                        const float* Ws, int Kb, int Cb, int N, const int32_t* n_dev, int act, const float* res,
                        int res_stride, const float* drop, float* out, void* stream) {
    return qt_dense2(a0, 0, a_rest, nullptr, 0, nullptr, Ka, Ca, 0, W, nullptr, S, Ks, Ws, Kb, Cb, 0, N, n_dev, act, res, res_stride, drop, out,
                     nullptr, 0, nullptr, nullptr, stream);
}

extern "C" int qt_wgrad_blocks(int N) { return N > 0 ? qt_cdiv(N, WGRAD_ROWS) : 0; }

extern "C" int qt_wgrad(const float* a0, int lda0, const float* a_rest, const float* a0b, int lda0b, const float* a_restb, int Ka,
                        int Ca, int Cab,
                        const float* S, int Ks, const float* G, int Co, int N, const int32_t* n_dev, int accumulate,
                        float* part, int planes_sm, void* stream) {
    QT_ARG(G && part && Co >= 1 && Co % 4 == 0 && ((uintptr_t)G & 15) == 0, "bad arguments");
    GemmArgs g = {};
    if (int rc = plane_src(&g.A, __func__, a0, lda0, a_rest, a0b, lda0b, a_restb, Ka, Ca, Cab, S, Ks, N, planes_sm)) return rc;
    if (N <= 0) return QT_OK;
    g.B = G; g.M = Ka * (Ca + Cab) + Ks; g.K = N; g.NB = Co;
    g.Kb = 1; g.Cb = Co; g.out = part; g.row0_step = WGRAD_ROWS; g.n_dev = n_dev; g.accumulate = accumulate;
    const dim3 grid(qt_cdiv(g.M, wgrad_fw(g.M) * 32), qt_cdiv(Co, BN), qt_cdiv(N, WGRAD_ROWS));
    QT_WGRAD_DISPATCH(k_gemm_wgrad, g.M, Co, grid, stream, g);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_wgrad_group_blocks(int nseg, const int* N) {
    int z = 0;
    for (int i = 0; i < nseg; ++i) z += N[i] > 0 ? qt_cdiv(N[i], WGRAD_ROWS) : 0;
    return z;
}

static int wgrad_group_launch(const char* fn, int nseg, const float* const* a0, const int* lda0, const float* const* a_rest,
                              const float* const* a0b, const int* lda0b, const float* const* a_restb, const float* const* S,
                              const float* const* G, const int* N, const int32_t* const* n_dev, int Ka, int Ca, int Cab, int Ks,
                              int Co, int ldg, int gpl, int Gn, int64_t gsA, int64_t gsG, int per_node, float* part, void* stream, int sm = 0) {
    WgradGroup w;
    w.sm = sm != 0;
    int z = 0, k = 0;
    for (int i = 0; i < nseg; ++i) {
        if (N[i] <= 0) continue;
        PlaneSrc A;
        if (int rc = plane_src(&A, fn, a0[i], lda0 ? lda0[i] : 0, Ka > 1 ? a_rest[i] : nullptr, Cab ? a0b[i] : nullptr,
                               (Cab && lda0b) ? lda0b[i] : 0, (Cab && Ka > 1) ? a_restb[i] : nullptr, Ka, Ca, Cab,
                               Ks ? S[i] : nullptr, Ks, N[i]))
            return rc;
        if (!G[i] || ((uintptr_t)G[i] & 15) != 0) {
            qt_set_error("%s: G must be 16-byte aligned", fn);
            return QT_E_ARG;
        }
        w.a0[k] = A.a0; w.a_rest[k] = A.a_rest; w.a0b[k] = A.a0b; w.a_restb[k] = A.a_restb; w.S[k] = A.S; w.G[k] = G[i];
        w.lda0[k] = A.lda0; w.lda0b[k] = A.lda0b;
        w.n_dev[k] = n_dev[i]; w.N[k] = N[i];
        z += qt_cdiv(N[i], WGRAD_ROWS);
        w.zend[k] = z;
        ++k;
    }
    if (k == 0) return QT_OK;
    for (int i = k; i < MAXSEG; ++i) {
        w.a0[i] = w.a_rest[i] = w.a0b[i] = w.a_restb[i] = w.S[i] = w.G[i] = nullptr;
        w.n_dev[i] = nullptr; w.N[i] = 0; w.zend[i] = z; w.lda0[i] = w.lda0b[i] = 0;
    }
    w.nseg = k; w.Ka = Ka; w.Ca = Ca; w.Cab = Cab; w.Ks = Ks; w.Co = Co; w.rows = WGRAD_ROWS; w.part = part;
    w.Gn = Gn; w.ytiles = qt_cdiv(Co, BN); w.ldg = ldg; w.gpl = gpl; w.gsA = gsA; w.gsG = gsG; w.per_node = per_node;
    const int M = Ka * (Ca + Cab) + Ks;
    const dim3 grid(qt_cdiv(M, wgrad_fw(M) * 32), w.ytiles * Gn, z);
    QT_WGRAD_DISPATCH(k_gemm_wgrad_group, M, Co, grid, stream, w);
    QT_LAUNCHED();
    return QT_OK;
}

extern "C" int qt_wgrad_group(int nseg, const float* const* a0, const int* lda0, const float* const* a_rest,
                              const float* const* a0b, const int* lda0b, const float* const* a_restb, const float* const* S, const float* const* G, const int* N,
                              const int32_t* const* n_dev, int Ka, int Ca, int Cab, int Ks, int Co, float* part, int planes_sm,
                              void* stream) {
    QT_ARG(nseg >= 1 && nseg <= MAXSEG && a0 && G && N && n_dev && part, "1..16 uses per launch");
    QT_ARG(Ka >= 1 && Ca >= 1 && Cab >= 0 && Co >= 1 && (Ka == 1 || a_rest) && (Ks == 0 || S) && (Cab == 0 || (a0b && (Ka == 1 || a_restb))),
           "bad arguments");
    QT_ARG(Co % 4 == 0, "Co must be a multiple of 4 (float4 operands)");
    return wgrad_group_launch(__func__, nseg, a0, lda0, a_rest, a0b, lda0b, a_restb, S, G, N, n_dev, Ka, Ca, Cab, Ks, Co, Co, 0, 1, 0, 0, 0,
                              part, stream, planes_sm);
}

// qt_wgrad_group for the Gn weights of qt_proj_group at once: use s multiplies [A_g | S]^T (A_g = a0[s] + g gsA, Cin columns,
// row stride lda0[s]) with the gradient rows G[s] + g gsG (Co columns, row stride ldg; gpl > 0: in Co / gpl planes (N[s], gpl)); per_node: gsA / gsG count floats per node (x N[s]).
// part: (qt_wgrad_group_blocks(nseg, N), Gn, Cin + Ks, Co), overwritten; qt_colsum over the blocks gives the (Gn, Cin + Ks, Co) gradient.
extern "C" int qt_wgrad_groups(int nseg, const float* const* a0, const int* lda0, const float* const* S, const float* const* G,
                               const int* N, const int32_t* const* n_dev, int Cin, int Ks, int Co, int ldg, int gpl, int Gn,
                               int64_t gsA, int64_t gsG, int per_node, float* part, void* stream) {
    QT_ARG(nseg >= 1 && nseg <= MAXSEG && a0 && lda0 && G && N && n_dev && part, "1..16 uses per launch");
    QT_ARG(Cin >= 4 && Co >= 4 && Co % 4 == 0 && (Ks == 0 || S) && Gn >= 1 && ldg % 4 == 0 && gsA % 4 == 0 && gsG % 4 == 0 &&
           (gpl ? (gpl % 4 == 0 && Co % gpl == 0 && ldg >= gpl) : ldg >= Co), "bad arguments");
    QT_ARG((int64_t)qt_cdiv(Co, BN) * Gn <= 65535, "too many groups");
    return wgrad_group_launch(__func__, nseg, a0, lda0, nullptr, nullptr, nullptr, nullptr, S, G, N, n_dev, 1, Cin, 0, Ks, Co, ldg, gpl, Gn,
                              gsA, gsG, per_node, part, stream);
}

extern "C" int qt_colsum(const float* part, int nblk, int64_t len, float* out, void* stream) {
    QT_ARG(part && out && len > 0 && nblk >= 0, "bad arguments");
    hipLaunchKernelGGL(k_colsum, dim3(qt_cdiv(len, 32)), dim3(1024), 0, (hipStream_t)stream, part, nblk, len, out);
    QT_LAUNCHED();
    return QT_OK;
}
