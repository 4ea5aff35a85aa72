// The row rule of the message aggregate  out = alpha L^ x + beta p + gamma q  of k_spmm, k_spmm1 (cheb.hip) and k_cheb_clip
// (chebclip.hip).  The arithmetic contract of the 4-CHANNEL rows (k_spmm at VEC = 4, k_cheb_clip), per row and channel:
//   acc = 0;  acc = fma(w_e, x[col_e], acc) for the ELL slots e = 0..3 (slots past the row's edges: weight 0), then for the
//   tail (edges 4, 5, .. of rows with more than four) in CSR order -- every step ONE fused multiply-add, spelled with the
//   intrinsic (vfma, fma4 below), so these kernels give the same sums because they run this text, not because the contraction
//   pass happens to fuse each of them alike.  Then  r = alpha acc (+ beta p) (+ gamma q).
// What is NOT covered by this header, each spelled out at its site because the shared form would change bits or the generated code:
//   * the SCALAR rows (k_spmm at VEC = 1, all of k_spmm1) sum separately rounded products w_e x -- multiply, then add, as the
//     compiler always emitted them -- so they agree with each other but not with a column of the 4-channel kernels;
//   * the finish: k_spmm's has one channel of four fused the other way round and the scalar rows' beta p unfused (cheb.hip says
//     which), k_cheb_clip's hop has r = alpha acc; r += A_k; r = fma(beta, own, r);
//   * k_cheb_clip decodes the ELL head and its two-int4 records itself and keeps its two pool walks (profiles/aggr_shared.txt).
#pragma once
#include "qt_common.h"

// the W channels of a slice row: a plain struct (independent registers: as one ext_vector value the 4-register tuples' alignment
// cost the W = 4 kernels ~25 more registers and spills); memory accesses go through the matching vector type
template <int W> struct fvec {
    float v[W];
    __device__ __forceinline__ float& operator[](int i) { return v[i]; }
    __device__ __forceinline__ const float& operator[](int i) const { return v[i]; }
};
template <int W> using fraw = float __attribute__((ext_vector_type(W)));
template <int W> __device__ __forceinline__ fvec<W> vload(const void* p) {
    const fraw<W> r = *reinterpret_cast<const fraw<W>*>(p);
    fvec<W> o;
#pragma unroll
    for (int i = 0; i < W; ++i) o.v[i] = r[i];
    return o;
}
template <int W> __device__ __forceinline__ void vstore(void* p, const fvec<W>& a) {
    fraw<W> r;
#pragma unroll
    for (int i = 0; i < W; ++i) r[i] = a.v[i];
    *reinterpret_cast<fraw<W>*>(p) = r;
}
template <int W> __device__ __forceinline__ fvec<W> vzero() {
    fvec<W> z;
#pragma unroll
    for (int i = 0; i < W; ++i) z.v[i] = 0.0f;
    return z;
}

// acc += w f, one fused multiply-add per channel.  Spelled with the intrinsic: left to the contraction pass, the vector form of
// w0 f0 + w1 f1 was fused the other way round in half the lanes -- 1 ulp away from the chain ((0 + w0 f0) + w1 f1) + ...
template <int W> __device__ __forceinline__ void vfma(fvec<W>& a, float w, const fvec<W>& f) {
#pragma unroll
    for (int i = 0; i < W; ++i) a[i] = __builtin_fmaf(w, f[i], a[i]);
}

// four edges: (((acc + w0 f0) + w1 f1) + w2 f2) + w3 f3
template <int W> __device__ __forceinline__ void fma4(fvec<W>& acc, const float* w, const fvec<W>* f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) vfma<W>(acc, w[e], f[e]);
}

// The first four edges of a row as the mesh build leaves them (qt_edges_norm: two int4 per row): columns, then the weights'
// bit patterns; a row with MORE than four edges is flagged by the complement of its last column.
struct EllHead {
    int4 c;
    float w[4];
    bool more;
};
__device__ __forceinline__ EllHead ell_head(int4 c, const int4& wb) {
    EllHead h;
    h.more = c.w < 0;
    if (h.more) c.w = ~c.w;
    h.c = c;
    h.w[0] = __int_as_float(wb.x);
    h.w[1] = __int_as_float(wb.y);
    h.w[2] = __int_as_float(wb.z);
    h.w[3] = __int_as_float(wb.w);
    return h;
}
__device__ __forceinline__ EllHead ell_head(const int4* __restrict__ ell, int64_t row) { return ell_head(ell[2 * row], ell[2 * row + 1]); }
