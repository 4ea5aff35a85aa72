// What the dense products (gemm.hip) and the gate-cell launches (gatecell.hip) both need: the node-feature operand and the
// argument block of the GEMM kernels, the tile constants, and the device helpers that address planes and rows.
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
    // gate GEMM with the LSTM cell as its epilogue (k_gemm_fwd<2, 128, true>): the (N, 4h) pre-activations never leave LDS
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

// Quad table: quad Q of a node row lives at qptr[Q] + row * qstr[Q] (plane Q*4/Ca of the operand, or S).
__device__ __forceinline__ void build_quad_table(const PlaneSrc& A, const float** qptr, int* qstr, int nquad) {
    for (int Q = threadIdx.x; Q < nquad; Q += 256) {
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
