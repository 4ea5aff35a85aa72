/*
 * qtmpnn_extent.h -- the regional ice extent / ice area entry of libqtmpnn_hip.so, declared beside qtmpnn.h (whose conventions,
 * error codes and qt_last_error() it shares) the way qtmpnn_edges.h declares qt_edge_rollout: the tests of the project hold
 * qtmpnn.h and its binding table to a fixed list of 87 entry points, so an entry added after them has its own header and its own
 * table (qtmpnn/_lib.py: _EXTENT_SIGNATURES).
 */
#ifndef QTMPNN_EXTENT_H
#define QTMPNN_EXTENT_H

#include "qtmpnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qt_extent_rollout: sea-ice extent, sea-ice area and the over- / under-forecast areas of a rollout per region, the sums behind
 * the integrated ice-edge error and its decomposition (Goessling et al. 2016: IIEE = O + U, AEE = |O - U|, ME = 2 min(O, U), all
 * three formed by the caller per forecast).  The arguments up to m, the sources (model: column 0 of the step's output through
 * the step's labels; then the dense baselines present, S = 1 + their number) and the counting rule are qt_score_rollout's.
 * Two per-pixel maps of n*m entries, shared by all clips and steps:
 *   region   int8 or NULL.  0 <= region[p] < R places pixel p in that region; any other value places it in none, and it adds
 *            nothing anywhere.  NULL: every pixel is in region 0.  R is in 1..32.
 *   area     float or NULL: the weight a of pixel p (a cell area).  NULL: 1.
 * With I_o = y > thr and I_s = f_s > thr (strict, fp32) the launch writes, per (step z, clip b, tile of 1024 pixels, region r),
 * 1 + S rows of 4 floats over the counted pixels of the region, partial[((((z*B + b)*ntile + tile)*R + r)*(1 + S) + row)*4 + slot]:
 *   row 0      the truth     slot 0  n (a count)      slot 1  A = sum a           slot 2  E_o = sum a I_o      slot 3  SIA_o = sum a y
 *   row 1 + s  source s      slot 0  E_s = sum a I_s  slot 1  SIA_s = sum a f_s   slot 2  O_s = sum a I_s (1 - I_o)
 *                                                                                 slot 3  U_s = sum a (1 - I_s) I_o
 * Grid (ceil(n*m/1024), B, nseg), 256 threads, one launch.  Summation order, fixed by pixel position: a thread adds its pixels p,
 * p + 256, p + 512, p + 768 of the tile that lie in the region in that order (a * y and a * f_s are rounded to fp32 once), then
 * the 64-lane butterfly (xor 32 .. 1), then (w0 + w1) + (w2 + w3) over the four waves; n is a popcount.  No atomics: the same
 * inputs give the same bits.  The caller adds the tiles (in float64: ops.rollout_extent).
 * NaN: a NaN forecast value is not ice (it counts as under-forecast where the truth is ice) and makes SIA_s of its own region,
 * tile and source NaN; it touches no count, no other slot, no other region and no other source.  A NaN truth is not ice and
 * makes SIA_o of its region and tile NaN, likewise.  The areas are the caller's to keep finite (ops.check_regions).
 * Refused with qt_last_error(): whatever qt_reliability_rollout refuses, an R outside 1..32 and a null partial. */
int qt_extent_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels, const int* Ns,
                      const int32_t* const* n_devs, const float* y, int64_t y_clip_stride, int64_t y_step_stride,
                      const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride, const float* base2,
                      int64_t base2_clip_stride, int64_t base2_step_stride, const uint8_t* pix_mask, float thr, int B, int n, int m,
                      const int8_t* region, const float* area, int R, float* partial, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QTMPNN_EXTENT_H */
