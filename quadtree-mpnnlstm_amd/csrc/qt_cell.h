// Device helpers of the peephole graph-LSTM cell shared by lstm.hip (stand-alone cell kernels), gemm.hip (the gate GEMM
// with the cell fused into its epilogue) and gatecell.hip (the persistent gate-cell launches): model/model.py:394-428 + the LayerNorms of model/seq2seq.py:64-75, 140-151.
// One copy each of what those kernels' bit-identity claims rest on: the cell arithmetic (cell_forward, cell_backward), its
// parameters (cell_params, cell_bwd_params), the backward's operand read (cell_bwd_load), the gate quarters (ld_gates,
// st_gates), the forward's stores (store_cell) and the fixed-order column sum of the parameter gradients (block_param_reduce).
#pragma once
#include "qt_common.h"

namespace qtcell {

constexpr float LN_EPS = 1e-5f;

// Branch-free gate nonlinearities on the hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32: 1 ulp each).  The libm forms
// (expf + IEEE division, tanhf with its range branches) cost ~25-40 instructions per value: 80 values per node made the
// cell ~10 us of pure VALU issue per launch at the bench shape, as much as the gate GEMM's MFMA time, and the branches
// kept the scheduler from placing that arithmetic beside the MFMAs.  Error, ABSOLUTE, from the instruction sequence (derived
// in tests/cell_f64.py: sig_own, tanh_own; u = 2^-24):
//   sigmoid  u [s (1 - s)(2 |x| + 2) + 3 s] <= 3.3 u = 2e-7.  Relative to s this is (1 - s)(2 |x| + 2) + 3 roundings: the rounding
//            of -log2(e) x is an absolute error of the exponent, so for negative x the relative error grows as |x| (5 ulp at
//            x = -2.5, 13 ulp at x = -10): "3 ulp" holds for x >= 0 only, and nothing may rest on a relative reading.
//   tanh     |x| >= 1/8: u [(1 - t^2)(2 |x| + 1) + 3 (1 - |t|) + |t|] <= 4 u = 2.4e-7, the most at |x| = 1/8, where it is
//            16 ulp of the result; |x| < 1/8 takes the odd series (the quotient form loses relative accuracy by cancellation):
//            (2 + x^2) u relative + 62 / 2835 |x|^9 for the series' end, under 2 ulp.
// A saturated argument is safe: exp2 overflows to inf, rcp(inf) = 0, so sigmoid -> 0 and tanh -> +-1 without a NaN.
// Forward and backward call the SAME functions, so recomputed values carry the same bits.
__device__ __forceinline__ float sigmoidf_(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float tanhf_(float x) {
    const float ax = fabsf(x), x2 = x * x;
    const float big = 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.8853900817779268f * ax));
    const float small = ax * fmaf(x2, fmaf(x2, fmaf(x2, -17.0f / 315.0f, 2.0f / 15.0f), -1.0f / 3.0f), 1.0f);
    return copysignf(ax < 0.125f ? small : big, x);
}

// v of lane l ^ D for the lane distances a DPP operand modifier can express (quad permutes for 1 and 2, a rotation of the
// 16-lane row by 8): the exchange rides on the add itself (v_add_f32_dpp), where __shfl_xor is a ds_bpermute_b32 -- an LDS
// instruction, its lane-index arithmetic and an lgkmcnt wait per step.  Same operands, same order: the same bits.  The
// source lane must be active (every lane of a node's group calls these together).
template <int D>
__device__ __forceinline__ float lane_xor(float v) {
    static_assert(D == 1 || D == 2 || D == 8, "no DPP control for this distance");
    constexpr int ctrl = D == 1 ? 0xB1 /* quad_perm:[1,0,3,2] */ : D == 2 ? 0x4E /* quad_perm:[2,3,0,1] */ : 0x128 /* row_ror:8 */;
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), ctrl, 0xf, 0xf, true));
}
// v of lane l + D of the same 16-lane row (row_shl:D; zero past the row's end)
template <int D>
__device__ __forceinline__ float lane_up(float v) {
    static_assert(D >= 1 && D <= 15, "row_shl:1 .. 15");
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x100 + D, 0xf, 0xf, true));
}

template <int LPN>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (LPN > 1) v += lane_xor<1>(v);
    if constexpr (LPN > 2) v += lane_xor<2>(v);
    if constexpr (LPN > 4) v += __shfl_xor(v, 4, 64);
    if constexpr (LPN > 8) v += lane_xor<8>(v);
#pragma unroll
    for (int d = 16; d < LPN; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct F4 {
    float v[4];
};
__device__ __forceinline__ F4 ld4(const float* p) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    return F4{{f.x, f.y, f.z, f.w}};
}
__device__ __forceinline__ void st4(float* p, const F4& a) {
    *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
}
// The four h-apart quarters of a gate row (pre-activations, activations or their gradients: i, f, c, o), p = row + j0
__device__ __forceinline__ void ld_gates(const float* p, int h, F4* a, F4* b, F4* c, F4* d) {
    *a = ld4(p); *b = ld4(p + h); *c = ld4(p + 2 * h); *d = ld4(p + 3 * h);
}
__device__ __forceinline__ void st_gates(float* p, int h, const F4& a, const F4& b, const F4& c, const F4& d) {
    st4(p, a); st4(p + h, b); st4(p + 2 * h, c); st4(p + 3 * h, d);
}

// y = gamma * xhat + beta over the group's h = 4 LPN values; returns xhat and rstd.  The means are products with the exact
// 1 / h (h is a power of two: the same bits as the IEEE division by a run-time h, which costs ~10 instructions each).
template <int LPN>
__device__ __forceinline__ void layer_norm(const F4& x, F4* xhat, float* rstd) {
    static_assert((LPN & (LPN - 1)) == 0, "1 / h must be exact");
    constexpr float inv_h = 1.0f / (4 * LPN);
    const float mean = group_sum<LPN>((x.v[0] + x.v[1]) + (x.v[2] + x.v[3])) * inv_h;
    float sq = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float d = x.v[k] - mean;
        sq += d * d;
    }
    const float var = group_sum<LPN>(sq) * inv_h;
    *rstd = 1.0f / sqrtf(var + LN_EPS);
#pragma unroll
    for (int k = 0; k < 4; ++k) xhat->v[k] = (x.v[k] - mean) * (*rstd);
}

// gx = rstd * (gxh - mean(gxh) - xhat * mean(gxh * xhat)),  gxh = gy * gamma
template <int LPN>
__device__ __forceinline__ F4 layer_norm_bwd(const F4& gy, const F4& gamma, const F4& xhat, float rstd) {
    constexpr float inv_h = 1.0f / (4 * LPN);
    F4 gxh;
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        gxh.v[k] = gy.v[k] * gamma.v[k];
        s1 += gxh.v[k];
        s2 += gxh.v[k] * xhat.v[k];
    }
    s1 = group_sum<LPN>(s1) * inv_h;
    s2 = group_sum<LPN>(s2) * inv_h;
    F4 gx;
#pragma unroll
    for (int k = 0; k < 4; ++k) gx.v[k] = rstd * (gxh.v[k] - s1 - xhat.v[k] * s2);
    return gx;
}

// C' before its LayerNorm.  The backward recomputes it from the saved gate activations instead of reading a saved copy, so
// the rounding is pinned here (one fma, not left to the compiler's contraction choice): both sides get the same bits.
__device__ __forceinline__ float cell_craw(float F, float cp, float I, float T) { return fmaf(F, cp, I * T); }

// One cell update for 4 hidden units of a node (this lane's slice j0 .. j0+3 of the h channels; the node's h/4 lanes are
// adjacent, LayerNorm statistics are shuffles inside that group -- every lane of the group must call this).
struct CellOut {
    F4 I, F, T, Og, Cr, hn, cn;
};
// The cell's parameters for this lane's 4 hidden units, loaded once (a persistent kernel keeps them in registers: a load in
// the epilogue would make the wave wait for every older load in its queue, the prefetched operand stream included).
struct CellParams {
    F4 wci, wcf, wco, bi, bf, bc, bo, gh, bh, gcn, bcn;
    bool has_ln;
};
__device__ __forceinline__ CellParams cell_params(const float* __restrict__ wc, const float* __restrict__ b,
                                                  const float* __restrict__ ln, int h, int j0) {
    CellParams p;
    p.wci = ld4(wc + j0); p.wcf = ld4(wc + h + j0); p.wco = ld4(wc + 2 * h + j0);
    p.bi = ld4(b + j0); p.bf = ld4(b + h + j0); p.bc = ld4(b + 2 * h + j0); p.bo = ld4(b + 3 * h + j0);
    p.has_ln = ln != nullptr;
    const F4 one = {{1, 1, 1, 1}}, zero = {{0, 0, 0, 0}};
    p.gh = p.gcn = one;
    p.bh = p.bcn = zero;
    if (ln) {
        p.gh = ld4(ln + j0); p.bh = ld4(ln + h + j0); p.gcn = ld4(ln + 2 * h + j0); p.bcn = ld4(ln + 3 * h + j0);
    }
    return p;
}

template <int LPN>
__device__ __forceinline__ CellOut cell_forward(const F4& gi, const F4& gf, const F4& gc, const F4& go, const F4& cp,
                                                const CellParams& P) {
    CellOut r;
    F4 Hr;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.I.v[k] = sigmoidf_(gi.v[k] + P.wci.v[k] * cp.v[k] + P.bi.v[k]);
        r.F.v[k] = sigmoidf_(gf.v[k] + P.wcf.v[k] * cp.v[k] + P.bf.v[k]);
        r.T.v[k] = tanhf_(gc.v[k] + P.bc.v[k]);
        r.Cr.v[k] = cell_craw(r.F.v[k], cp.v[k], r.I.v[k], r.T.v[k]);
        r.Og.v[k] = sigmoidf_(go.v[k] + P.wco.v[k] * r.Cr.v[k] + P.bo.v[k]);
        Hr.v[k] = r.Og.v[k] * tanhf_(r.Cr.v[k]);
    }
    r.hn = Hr;
    r.cn = r.Cr;
    if (P.has_ln) {
        F4 xh, xc;
        float rh, rc;
        layer_norm<LPN>(Hr, &xh, &rh);
        layer_norm<LPN>(r.Cr, &xc, &rc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r.hn.v[k] = P.gh.v[k] * xh.v[k] + P.bh.v[k];
            r.cn.v[k] = P.gcn.v[k] * xc.v[k] + P.bcn.v[k];
        }
    }
    return r;
}

template <int LPN>
__device__ __forceinline__ CellOut cell_forward(const F4& gi, const F4& gf, const F4& gc, const F4& go, const F4& cp,
                                                const float* __restrict__ wc, const float* __restrict__ b,
                                                const float* __restrict__ ln, int h, int j0) {
    return cell_forward<LPN>(gi, gf, gc, go, cp, cell_params(wc, b, ln, h, j0));
}

// The forward's stores for this lane's 4 hidden units of `node`: O (the output gate once more, NULL: skipped), H', C' and the
// gate activations the backward reads (NULL: a forward-only launch).  k_lstm_fwd, k_gemm_fwd's CELL epilogue and
// k_gate_cell_p all store through this.
__device__ __forceinline__ void store_cell(float* O, float* Hn, float* Cn, float* gates, int64_t node, int h, int j0,
                                           const CellOut& r) {
    if (O) st4(O + node * h + j0, r.Og);
    st4(Hn + node * h + j0, r.hn);
    st4(Cn + node * h + j0, r.cn);
    if (gates) st_gates(gates + node * 4 * h + j0, h, r.I, r.F, r.T, r.Og);
}

// The backward's parameters for this lane's 4 hidden units (gamma = 1 without LayerNorm), as CellParams for the forward.
struct CellBwdParams {
    F4 wci, wcf, wco, gam_h, gam_c;
    bool has_ln;
};
__device__ __forceinline__ CellBwdParams cell_bwd_params(const float* __restrict__ wc, const float* __restrict__ ln, int h, int j0) {
    CellBwdParams p;
    p.wci = ld4(wc + j0); p.wcf = ld4(wc + h + j0); p.wco = ld4(wc + 2 * h + j0);
    p.has_ln = ln != nullptr;
    const F4 one = {{1, 1, 1, 1}};
    p.gam_h = p.gam_c = one;
    if (ln) {
        p.gam_h = ld4(ln + j0);
        p.gam_c = ld4(ln + 2 * h + j0);
    }
    return p;
}

// The backward's operands for this lane's 4 hidden units of `node`: the saved gate activations, C, and the gradients of
// H', C' and O.  A null pointer gives zeros (no previous state; an output nobody used has no gradient), and so does every
// operand of a row that is not ok (past the valid count).  gHn2: an optional second gradient of H', added on load.
struct CellBwdIn {
    F4 I, F, T, Og, cp, gyh, gyc, go_in;
};
__device__ __forceinline__ CellBwdIn cell_bwd_load(bool ok, int64_t node, int h, int j0, const float* gates, const float* Cprev,
                                                   int ld_c, const float* gHn, int ld_gh, const float* gCn, int ld_gc,
                                                   const float* gO, int ld_go, const float* gHn2 = nullptr, int ld_gh2 = 0) {
    const F4 z = {{0, 0, 0, 0}};
    CellBwdIn x = {z, z, z, z, z, z, z, z};
    if (ok) {
        ld_gates(gates + node * 4 * h + j0, h, &x.I, &x.F, &x.T, &x.Og);
        if (Cprev) x.cp = ld4(Cprev + node * ld_c + j0);
        if (gHn) x.gyh = ld4(gHn + node * ld_gh + j0);
        if (gCn) x.gyc = ld4(gCn + node * ld_gc + j0);
        if (gO) x.go_in = ld4(gO + node * ld_go + j0);
        if (gHn2) {
            const F4 h2 = ld4(gHn2 + node * ld_gh2 + j0);
#pragma unroll
            for (int k = 0; k < 4; ++k) x.gyh.v[k] += h2.v[k];
        }
    }
    return x;
}

// Backward of one cell update for 4 hidden units of a node (lane group as in cell_forward).  acc[11][4] collects this
// thread's parameter-gradient terms: w_c i, f, o | b i, f, c, o | LayerNorm gamma_h, beta_h, gamma_c, beta_c.
struct CellBwdOut {
    F4 ggi, ggf, ggc, ggo, gcp;
};
template <int LPN>
__device__ __forceinline__ CellBwdOut cell_backward(const CellBwdIn& x, const CellBwdParams& P, float (&acc)[11][4]) {
    const F4 &I = x.I, &F = x.F, &T = x.T, &Og = x.Og, &cp = x.cp, &gyh = x.gyh, &gyc = x.gyc, &go_in = x.go_in;
    const F4 &wci = P.wci, &wcf = P.wcf, &wco = P.wco, &gam_h = P.gam_h, &gam_c = P.gam_c;
    const bool has_ln = P.has_ln;
    F4 Cr, Hr, tc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        Cr.v[k] = cell_craw(F.v[k], cp.v[k], I.v[k], T.v[k]);        // not saved by the forward: same fma, same bits
        tc.v[k] = tanhf_(Cr.v[k]);
        Hr.v[k] = Og.v[k] * tc.v[k];
    }
    F4 xh = {{0, 0, 0, 0}}, xc = {{0, 0, 0, 0}};
    F4 gHr = gyh, gCr = gyc;
    if (has_ln) {
        float rh, rc;
        layer_norm<LPN>(Hr, &xh, &rh);
        layer_norm<LPN>(Cr, &xc, &rc);
        gHr = layer_norm_bwd<LPN>(gyh, gam_h, xh, rh);
        gCr = layer_norm_bwd<LPN>(gyc, gam_c, xc, rc);
    }
    CellBwdOut o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        acc[7][k] += gyh.v[k] * xh.v[k];
        acc[8][k] += gyh.v[k];
        acc[9][k] += gyc.v[k] * xc.v[k];
        acc[10][k] += gyc.v[k];
        const float gOt = go_in.v[k] + gHr.v[k] * tc.v[k];
        float gc_ = gCr.v[k] + gHr.v[k] * Og.v[k] * (1.0f - tc.v[k] * tc.v[k]);
        o.ggo.v[k] = gOt * Og.v[k] * (1.0f - Og.v[k]);
        gc_ += o.ggo.v[k] * wco.v[k];
        o.ggi.v[k] = gc_ * T.v[k] * I.v[k] * (1.0f - I.v[k]);
        o.ggf.v[k] = gc_ * cp.v[k] * F.v[k] * (1.0f - F.v[k]);
        o.ggc.v[k] = gc_ * I.v[k] * (1.0f - T.v[k] * T.v[k]);
        o.gcp.v[k] = gc_ * F.v[k] + o.ggi.v[k] * wci.v[k] + o.ggf.v[k] * wcf.v[k];
        acc[0][k] += o.ggi.v[k] * cp.v[k];
        acc[1][k] += o.ggf.v[k] * cp.v[k];
        acc[2][k] += o.ggo.v[k] * Cr.v[k];
        acc[3][k] += o.ggi.v[k];
        acc[4][k] += o.ggf.v[k];
        acc[5][k] += o.ggc.v[k];
        acc[6][k] += o.ggo.v[k];
    }
    return o;
}

// Sum over a wave of the values that lanes LPN apart hold (the same hidden units of the wave's 64 / LPN nodes); the result is
// valid in lanes 0 .. LPN-1 only.  The additions are those of the xor butterfly (v[l] + v[l ^ d], d = LPN, 2 LPN, .. 32) as
// lanes < LPN see it; inside a 16-lane row the partner comes through DPP (lane l + d: what l ^ d is for the lanes that
// count), across rows through ds_bpermute.
template <int LPN>
__device__ __forceinline__ float wave_strided_sum(float v) {
    if constexpr (LPN <= 1) v += lane_up<1>(v);
    if constexpr (LPN <= 2) v += lane_up<2>(v);
    if constexpr (LPN <= 4) v += lane_up<4>(v);
    if constexpr (LPN <= 8) v += lane_up<8>(v);
#pragma unroll
    for (int d = (LPN > 16 ? LPN : 16); d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// reduce NACC*4 per-thread accumulators over a workgroup of NW waves into part_row[NACC * h]; sm: NW * LPN * NACC * 4 floats.
// Every thread of the workgroup calls it.  The barrier waits for LDS only, which is enough for every caller: `sm` is written
// and read nowhere else, and part_row[idx] is read and written by one thread.
template <int LPN, int NACC, int NW = 4>
__device__ __forceinline__ void block_param_reduce(float (&acc)[NACC][4], int h, float* sm, float* part_row, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NACC; ++a)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[a][k] = wave_strided_sum<LPN>(acc[a][k]);
    if (lane < LPN) {
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int k = 0; k < 4; ++k) sm[(wave * LPN + lane) * NACC * 4 + a * 4 + k] = acc[a][k];
    }
    qt_lds_barrier();                      // (only `sm` crosses: the rows' global stores issued before stay in flight)
    for (int idx = threadIdx.x; idx < NACC * h; idx += 64 * NW) {
        const int a = idx / h, j = idx % h;
        const int li = j >> 2, k = j & 3;
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) s += sm[(w * LPN + li) * NACC * 4 + a * 4 + k];
        part_row[idx] = accumulate ? part_row[idx] + s : s;
    }
}

}  // namespace qtcell
