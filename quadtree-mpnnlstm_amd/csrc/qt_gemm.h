// What the dense products (gemm.hip) and the gate-cell launches (gatecell.hip) both need: the node-feature operand and the
// argument block of the GEMM kernels, the tile constants, the device helpers that address planes and rows, and the pieces the
// dense kernels share: act_quad / relu_bwd_quad, fma_quad / post_product, store_split and stage_and_store (cheb.hip's
// k_spmm1 takes act_quad from here too); and what every fp32 MFMA kernel of gemm.hip, gatecell.hip and projbwd.hip shares: the
// four-MFMA step of a k-quad (mfma_quad), the accumulator row map (acc_row) and the quad table (build_quad_table).
#pragma once
#include "qt_common.h"

// (in the anonymous namespace like the kernels that take them: the argument structs are part of the kernels' names)
namespace {

// ------------------------------------------------------------------ tiled GEMM
// Node-feature operand made of Ka planes plus an optional (N, Ks) block.  A plane is one (N, Ca) matrix or two matrices side
// by side, (N, Ca) | (N, Cab): the recurrent cells feed Z = [X | H] without ever concatenating it -- rows of 64 bytes (H)
// and 16 bytes (X) also keep every 4-lane group of a gather inside one row, which rows of 80 bytes do not.
struct PlaneSrc {
    const float* a0;        // plane 0, part a (N, Ca)
    const float* a_rest;    // planes 1 .. Ka-1, part a (Ka-1, N, Ca)
    const float* a0b;       // part b of the same planes: (N, Cab) and (Ka-1, N, Cab); Cab == 0: none
    const float* a_restb;
    const float* S;
    int Ka, Ca, Cab, Ks, N;
    int lda0, lda0b;        // row strides of plane 0 (column views of wider matrices are passed as they are)
    int sm;                 // planes 1 .. Ka-1 are stored SLICE-major: (plane, 4-channel slice, N, 4) -- the layout the clip-resident
                            // recurrence writes (consecutive rows of a slice are contiguous: coalesced stores there, and a quad of a
                            // row is reached at slice base + row * 4 here)
};

struct GemmArgs {
    PlaneSrc A;        // forward: left operand rows = nodes; wgrad: transposed use
    const float* B;    // forward: W (K, NB); wgrad: G (N, NB)
    const float* BT;   // forward, optional: W^T (NB, K) -- staged with straight float4 copies instead of a transposing scatter
    int M, K, NB;      // output M x NB, reduction K
    // forward epilogue
    int Kb, Cb, act;
    const float* res;
    int res_stride;
    const float* drop;
    float* out;
    float* outb;        // forward: second column part of every output plane, (Kb, M, Cbb); Cbb == 0: none
    int Cbb;
    int out_sm;         // output planes 1 .. Kb-1 slice-major (plane_piece)
    // k_gemm_skinny<64> with NB = 16: a second product in the epilogue, post_out (M, 4) = [act(out) | 1 0 0 0] @ post_W (NB + 4, 4)
    // (the decoder head: fc_out1's 16 channels -> the three coefficient columns of fc_out2, seq2seq.py:115-121)
    const float* post_W;
    float* post_out;
    int64_t row0_step;  // wgrad: rows per block
    const int32_t* n_dev;  // valid node rows on the device (NULL: A.N)
    int accumulate;        // wgrad: add into part instead of overwriting (sums several uses of one weight)
    // gate GEMM with the LSTM cell as its epilogue (k_gemm_fwd<NT, KWT, CELL = h / 4>): the (N, 4h) pre-activations never leave LDS
    const float* Cprev;
    const float* wc;
    const float* bias;
    const float* ln;
    int ld_c, h;
    float *O, *Hn, *Cn, *gates;
    // grouped use (qt_proj_group): blockIdx.z = group; plane 0, the weight and the output of group z start gsA / gsB / gsO
    // floats after those of group z - 1.  ldo: row stride of the output plane (0 = Cb; a column block of a wider matrix)
    int ldo, zrev;
    int64_t gsA, gsB, gsO;
};

// ---- fp32 MFMA tiles (v_mfma_f32_32x32x2_f32: exact fp32 fma chain, 64 FLOP/clk/SIMD).
// Operand maps (cdna_hip_programming.md section 3): lane l holds A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31]; accumulator register r of lane l is C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].
// The two k slots of one MFMA may be ANY two reduction indices as long as A and B agree, which is what lets a
// lane fetch its A operand as one float4 (4 consecutive k of its own row): in step (j, i) lane half h feeds
// k = 8 j + 4 h + i.
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int BM = 128;       // block rows (4 waves x 32)
constexpr int BN = 64;        // block columns (2 MFMA tiles per wave)
constexpr int MAXQ = 128;     // quads (4 consecutive k) in the reduction dimension

// Row of the 32 x 32 tile that accumulator register r of a lane of half (lane >> 5) holds
__device__ __forceinline__ constexpr int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// One k-quad of a lane on one column tile: the four MFMAs on a.x .. a.w with b.x .. b.w, in that order
__device__ __forceinline__ void mfma_quad(f32x16& acc, const float4& a, const float4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
}

// Pointers that went through the LDS quad table lose their address space: hipcc then emits flat_load, and flat loads
// force `s_waitcnt vmcnt(0) lgkmcnt(0)` at every use (they may return out of order), which serialised the whole
// operand stream.  Loading through an explicit global (address space 1) pointer restores counted vmcnt waits.
typedef float qt_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 gload4(const float* p) {
    const qt_v4f v = *(const __attribute__((address_space(1))) qt_v4f*)p;
    return make_float4(v.x, v.y, v.z, v.w);
}

// float4 piece (plane pl, row i, channel ch) of an OUTPUT plane set of width C: row-major (planes, M, C) -- or, with sm, planes
// 1.. slice-major (C / 4, M, 4), the layout the clip-resident Clenshaw launch reads with coalesced loads (plane 0 stays row-major:
// it becomes the gradient matrix of the layer's input)
__device__ __forceinline__ float* plane_piece(float* base, int pl, int64_t i, int ch, int C, int64_t M, int sm, int ld) {
    if (sm && pl > 0) return base + (((int64_t)pl * (C >> 2) + (ch >> 2)) * M + i) * 4;
    return base + (int64_t)pl * M * C + i * ld + ch;
}

// ---- the arithmetic and the stores that several dense kernels share.  One copy each: the kernels' bit-identity claims
// ("the same fused multiply-adds in the same order as ...") rest on these staying the same everywhere.

// Epilogue activation: QT_ACT_RELU = max(d v, 0), QT_ACT_TANH_RES = tanh(d v) + rs, d = the row's dropout factor (a row
// without a mask passes 1.0f: x 1.0f is exact, the same bits), rs = the row's residual.  Any other act: v unchanged.
__device__ __forceinline__ float act_quad(float v, int act, float d, float rs) {
    if (act == QT_ACT_RELU) return fmaxf(d * v, 0.0f);
    if (act == QT_ACT_TANH_RES) return tanhf(d * v) + rs;
    return v;
}
__device__ __forceinline__ float4 act_quad(float4 v, int act, float d, float rs) {
    if (act == QT_ACT_RELU) v = make_float4(fmaxf(d * v.x, 0.0f), fmaxf(d * v.y, 0.0f), fmaxf(d * v.z, 0.0f), fmaxf(d * v.w, 0.0f));
    if (act == QT_ACT_TANH_RES) v = make_float4(tanhf(d * v.x) + rs, tanhf(d * v.y) + rs, tanhf(d * v.z) + rs, tanhf(d * v.w) + rs);
    return v;
}
// QT_ACT_RELU_BWD: v * relu'(y), y = the forward output
__device__ __forceinline__ float4 relu_bwd_quad(float4 v, float4 y) {
    return make_float4(y.x > 0.0f ? v.x : 0.0f, y.y > 0.0f ? v.y : 0.0f, y.z > 0.0f ? v.z : 0.0f, y.w > 0.0f ? v.w : 0.0f);
}

// acc (4 output columns) += a (4 consecutive k) x the 4 x 4 block of W whose rows start at W, ldw apart: sixteen fused multiply-adds, k ascending
__device__ __forceinline__ void fma_quad(float4& acc, const float4& a, const float* __restrict__ W, int64_t ldw) {
    const float4 w0 = *reinterpret_cast<const float4*>(W);
    const float4 w1 = *reinterpret_cast<const float4*>(W + ldw);
    const float4 w2 = *reinterpret_cast<const float4*>(W + 2 * ldw);
    const float4 w3 = *reinterpret_cast<const float4*>(W + 3 * ldw);
    acc.x = fmaf(a.x, w0.x, acc.x); acc.y = fmaf(a.x, w0.y, acc.y); acc.z = fmaf(a.x, w0.z, acc.z); acc.w = fmaf(a.x, w0.w, acc.w);
    acc.x = fmaf(a.y, w1.x, acc.x); acc.y = fmaf(a.y, w1.y, acc.y); acc.z = fmaf(a.y, w1.z, acc.z); acc.w = fmaf(a.y, w1.w, acc.w);
    acc.x = fmaf(a.z, w2.x, acc.x); acc.y = fmaf(a.z, w2.y, acc.y); acc.z = fmaf(a.z, w2.z, acc.z); acc.w = fmaf(a.z, w2.w, acc.w);
    acc.x = fmaf(a.w, w3.x, acc.x); acc.y = fmaf(a.w, w3.y, acc.y); acc.z = fmaf(a.w, w3.z, acc.z); acc.w = fmaf(a.w, w3.w, acc.w);
}
// The decoder head's second product, (4 columns) = [q[0] .. q[3] | 1 0 0 0] @ post_W (20, 4): the fused multiply-adds, in the
// order, of a k_gemm_skinny<256> launch on the stored 16-column row (quads 0 .. 3, then the bias quad)
__device__ __forceinline__ float4 post_product(const float4 (&q)[4], const float* __restrict__ post_W) {
    float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int Q = 0; Q <= 4; ++Q) fma_quad(u, Q < 4 ? q[Q] : make_float4(1.f, 0.f, 0.f, 0.f), post_W + 16 * Q, 4);
    return u;
}

// float4 v = columns j .. j + 3 of output row i: to its plane and part (out | outb; Cb, Cbb % 4 == 0: a float4 never straddles
// two parts).  ld: the row stride of part a (g.Cb, or g.ldo for a column block of a wider matrix).  add0: optional (M, Cb),
// added to plane 0 of part a.  On plain fields for the kernels whose argument block is not a GemmArgs.
__device__ __forceinline__ void store_split(float* out, float* outb, int Cb, int Cbb, int M, int out_sm, int j, int64_t i,
                                            float4 v, int ld, const float* add0 = nullptr) {
    const int ct = Cb + Cbb;
    const int pl = j / ct, ch = j - pl * ct;
    if (ch < Cb) {
        if (pl == 0 && add0) {
            const float4 e = *reinterpret_cast<const float4*>(add0 + i * Cb + ch);
            v.x += e.x; v.y += e.y; v.z += e.z; v.w += e.w;
        }
        *reinterpret_cast<float4*>(plane_piece(out, pl, i, ch, Cb, M, out_sm, ld)) = v;
    } else {
        *reinterpret_cast<float4*>(plane_piece(outb, pl, i, ch - Cb, Cbb, M, out_sm, Cbb)) = v;
    }
}
__device__ __forceinline__ void store_split(const GemmArgs& g, int j, int64_t i, float4 v, int ld) {
    store_split(g.out, g.outb, g.Cb, g.Cbb, g.M, g.out_sm, j, i, v, ld);
}

// The staged epilogue of the MFMA kernels (256 threads, wave w owns rows [32 w, 32 w + 32) of the 128 x 32 NT tile at (i0, j0)).
// An MFMA accumulator holds one COLUMN per lane; staging the tile in LDS (Cs: BM x 64 floats, the W buffer, free by now) lets
// every thread write float4 pieces of output ROWS instead (4x fewer, 16-byte wide, row-contiguous stores).  Two 32-column MFMA
// tiles per pass (the last pass of an odd NT: one).  Every thread of the workgroup must call it: both barriers of a pass are
// outside any divergent code.
template <int NT>
__device__ __forceinline__ void stage_and_store(f32x16 (&acc)[NT], float* Cs, const GemmArgs& g, int64_t i0, int j0, int64_t rows) {
    const int t = threadIdx.x, wave = t >> 6, l32 = t & 31, half = (t >> 5) & 1;
    const int ld = g.ldo ? g.ldo : g.Cb;
#pragma unroll
    for (int h2 = 0; h2 < (NT + 1) / 2; ++h2) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int nt = 2 * h2 + u;
            if (nt < NT)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    Cs[(wave * 32 + acc_row(r, half)) * 64 + u * 32 + l32] = acc[nt][r];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < BM * 16 / 256; ++u) {
            const int e = t + 256 * u;
            const int row = e >> 4, c4 = (e & 15) * 4;
            const int64_t i = i0 + row;
            const int j = j0 + h2 * 64 + c4;
            if (i >= rows || j >= g.NB || h2 * 64 + c4 >= 32 * NT) continue;
            float4 v = *reinterpret_cast<const float4*>(&Cs[row * 64 + c4]);
            // (a call per activation: g.drop and g.res are read only under the test that needs them -- res may be null otherwise)
            if (g.act == QT_ACT_RELU) v = act_quad(v, QT_ACT_RELU, g.drop ? g.drop[i] : 1.0f, 0.0f);
            if (g.act == QT_ACT_TANH_RES) v = act_quad(v, QT_ACT_TANH_RES, g.drop ? g.drop[i] : 1.0f, g.res[i * g.res_stride]);
            store_split(g, j, i, v, ld);
        }
    }
}

// Quad table: quad Q of a node row lives at qptr[Q] + row * qstr[Q] (plane Q*4/Ca of the operand, or S).  NTHR: the threads of
// the calling workgroup.
template <int NTHR = 256>
__device__ __forceinline__ void build_quad_table(const PlaneSrc& A, const float** qptr, int* qstr, int nquad) {
    for (int Q = threadIdx.x; Q < nquad; Q += NTHR) {
        const int ct = A.Ca + A.Cab;
        const int k = 4 * Q, kc = A.Ka * ct;
        if (k < kc) {
            const int pl = k / ct, c = k - pl * ct;
            if (c < A.Ca) {
                if (pl > 0 && A.sm) {
                    qptr[Q] = A.a_rest + ((int64_t)(pl - 1) * (A.Ca / 4) + c / 4) * A.N * 4;
                    qstr[Q] = 4;
                } else {
                    qptr[Q] = (pl == 0 ? A.a0 : A.a_rest + (int64_t)(pl - 1) * A.N * A.Ca) + c;
                    qstr[Q] = pl == 0 ? A.lda0 : A.Ca;
                }
            } else {
                if (pl > 0 && A.sm) {
                    qptr[Q] = A.a_restb + ((int64_t)(pl - 1) * (A.Cab / 4) + (c - A.Ca) / 4) * A.N * 4;
                    qstr[Q] = 4;
                } else {
                    qptr[Q] = (pl == 0 ? A.a0b : A.a_restb + (int64_t)(pl - 1) * A.N * A.Cab) + (c - A.Ca);
                    qstr[Q] = pl == 0 ? A.lda0b : A.Cab;
                }
            }
        } else {
            qptr[Q] = A.S + (k - kc);
            qstr[Q] = A.Ks;
        }
    }
}

}  // namespace

// shared argument checks / operand setup of the node-feature operand
static inline int plane_src(PlaneSrc* A, const char* fn, const float* a0, int lda0, const float* a_rest, const float* a0b, int lda0b,
                            const float* a_restb, int Ka, int Ca, int Cab, const float* S, int Ks, int N, int sm = 0) {
    const bool ok = a0 && Ka >= 1 && Ca >= 1 && Cab >= 0 && (Ka == 1 || a_rest) && (Cab == 0 || (a0b && (Ka == 1 || a_restb))) &&
                    (Ks == 0 || S) && Ca % 4 == 0 && Cab % 4 == 0 && Ks % 4 == 0 && lda0 % 4 == 0 && lda0b % 4 == 0 && (Ka * (Ca + Cab) + Ks) / 4 <= MAXQ &&
                    (((uintptr_t)a0 | (uintptr_t)a_rest | (uintptr_t)a0b | (uintptr_t)a_restb | (uintptr_t)S) & 15) == 0;
    if (!ok) {
        qt_set_error("%s: bad node-feature operand (planes / parts must be 16-byte aligned with widths that are multiples of 4, "
                     "reduction dimension <= 512)", fn);
        return QT_E_ARG;
    }
    A->a0 = a0; A->a_rest = a_rest; A->a0b = Cab ? a0b : nullptr; A->a_restb = Cab ? a_restb : nullptr; A->S = S;
    A->Ka = Ka; A->Ca = Ca; A->Cab = Cab; A->Ks = Ks; A->N = N;
    A->lda0 = lda0 > 0 ? lda0 : Ca; A->lda0b = lda0b > 0 ? lda0b : Cab;
    A->sm = sm != 0;
    return QT_OK;
}

// The gate GEMM with the LSTM cell as its epilogue, k_gemm_fwd<.., CELL> (gemm.hip, its only instantiation), for the
// branch of qt_dense_lstm (gatecell.hip) that the persistent kernel does not cover.  `gemm_args` points to a filled GemmArgs: a
// type of the anonymous namespace cannot appear in a signature that two files link through.  Not part of the C ABI.
__attribute__((visibility("hidden"))) void gemm_fwd_cell_launch(const void* gemm_args, int N, hipStream_t stream);
