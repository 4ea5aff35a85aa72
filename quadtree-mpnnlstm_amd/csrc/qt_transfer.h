// What the mesh <-> image transfer kernels of transfer.hip and remeshclip.hip share, each rule written once: the parts table of
// a state that is several matrices side by side, the small vector types, the pyramid sum and the width dispatch.
#pragma once
#include "qt_common.h"

namespace qttransfer {

// One side of a state transfer: up to 8 matrices side by side, rows of ld[i] floats, widths as float4 prefix sums end[i].  The
// source side (T = const float, row-strided parts welcome) and the result side (T = float, dense rows: ld = width, so that every
// consumer reads dense rows) are the same table; PoolArgs and RcArgs hold one of each.
template <class T> struct PartTable {
    T* p[8];
    int ld[8], end[8];
};

// A PartTable checked and filled: n matrices ptrs[i] of widths[i] floats with row stride lds[i] (lds == NULL: dense rows).
// Returns the width in float4 chunks, or -1 with the error set to "fn: msg" (the caller's own text).  The entries past n end
// at 2^30: no chunk index reaches them.
template <class T>
inline int fill_parts(const char* fn, const char* msg, T* const* ptrs, const int* widths, const int* lds, int n, PartTable<T>& t) {
    int c4 = 0;
    for (int i = 0; i < n; ++i) {
        const int l = lds ? lds[i] : widths[i];
        if (!(ptrs[i] && widths[i] > 0 && widths[i] % 4 == 0 && l % 4 == 0 && l >= widths[i] && ((uintptr_t)ptrs[i] & 15) == 0)) {
            qt_set_error("%s: %s", fn, msg);
            return -1;
        }
        t.p[i] = ptrs[i];
        t.ld[i] = l;
        c4 += widths[i] / 4;
        t.end[i] = c4;
    }
    for (int i = n; i < 8; ++i) { t.p[i] = nullptr; t.ld[i] = 0; t.end[i] = 1 << 30; }
    return c4;
}

// address of float4 chunk `ch` of row `row` (*ld, if asked for: the row stride of the chunk's part)
template <class T> __device__ __forceinline__ T* part_chunk(const PartTable<T>& t, int64_t row, int ch, int* ld = nullptr) {
    int s = 0;
    while (ch >= t.end[s]) ++s;
    if (ld) *ld = t.ld[s];
    return t.p[s] + row * t.ld[s] + (ch - (s ? t.end[s - 1] : 0)) * 4;
}

// VEC channels of a row: a float4 chunk, or one float where the width or the alignment rules float4 out
template <int VEC> struct Vec { float v[VEC]; };
template <int VEC> __device__ __forceinline__ Vec<VEC> vload(const float* p) {
    Vec<VEC> r;
    if constexpr (VEC == 4) {
        const float4 f = *reinterpret_cast<const float4*>(p);
        r.v[0] = f.x; r.v[1] = f.y; r.v[2] = f.z; r.v[3] = f.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int VEC> __device__ __forceinline__ void vstore(float* p, const Vec<VEC>& r, float scale) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = r.v[k] * scale;
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 mul4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// The pyramid sum, the order every transfer is held to: (top-left + top-right) + (bottom-left + bottom-right)
__device__ __forceinline__ float quad_add(float a, float b, float c, float d) { return (a + b) + (c + d); }
__device__ __forceinline__ float4 quad_add(float4 a, float4 b, float4 c, float4 d) { return add4(add4(a, b), add4(c, d)); }
template <int VEC> __device__ __forceinline__ Vec<VEC> quad_add(const Vec<VEC>& a, const Vec<VEC>& b, const Vec<VEC>& c, const Vec<VEC>& d) {
    Vec<VEC> r;
#pragma unroll
    for (int k = 0; k < VEC; ++k) r.v[k] = quad_add(a.v[k], b.v[k], c.v[k], d.v[k]);
    return r;
}

}  // namespace qttransfer

// Launches KERNEL<4> where rows move as float4 chunks (v4) and KERNEL<1> otherwise
#define QT_TRANSFER_LAUNCH(v4, KERNEL, grid, block, stream, ...)                                                      \
    do {                                                                                                              \
        if (v4) hipLaunchKernelGGL(KERNEL<4>, dim3(grid), dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);          \
        else hipLaunchKernelGGL(KERNEL<1>, dim3(grid), dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);             \
    } while (0)
