/*
 * qtmpnn_edges.h -- the ice-edge verification entry of libqtmpnn_hip.so, declared beside qtmpnn.h (whose conventions, error
 * codes and qt_last_error() it shares): the tests of the project hold qtmpnn.h and its binding table to a fixed list of 87
 * entry points, so an entry added after them has its own header and its own table (qtmpnn/_lib.py: _EDGE_SIGNATURES).
 */
#ifndef QTMPNN_EDGES_H
#define QTMPNN_EDGES_H

#include "qtmpnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* qt_edge_rollout: ice-edge displacement of a rollout (average ice-edge displacement and Hausdorff distances, Dukhovskoy et
 * al. 2015, Melsom et al. 2019), all in integers.  The arguments up to m, the sources (model: column 0 of the step's output
 * through the step's labels; then the dense baselines present) and the counting rule are qt_score_rollout's; the frame is n rows
 * of m pixels, p = r*m + c, at most 256 x 256 (a larger frame is refused: the search keeps a frame's edge sets in LDS).
 *   counted(p)   the step's label lab has 0 <= lab < rows and p is not under pix_mask.
 *   ice(x, p)    counted(p) && x[p] > thr, strict, fp32: NaN and -inf are not ice, +inf is.
 *   E(x)         the edge set of field x: the pixels p with ice(x, p) that have at least one 4-neighbour which is inside the
 *                frame, counted, and not ice.  Frame borders and uncounted pixels (land, mask, no node) make no edge.
 *   d2(p, E)     for a non-empty set E, min over e in E of dr^2 + dc^2: exact over the whole frame, no search radius.
 *   q(p, E)      isqrt(65536 * d2(p, E)): the distance in 1/256 pixel, rounded down, exact (fixed up in 64-bit integers).
 * Grid (ceil(n/16), B, nseg), two launches: the first leaves E(y) and E(f_s) as bit-planes in `planes`, scratch of
 * nseg * B * (S + 1) * n * ceil(m/64) 64-bit words that the caller provides and need not initialise; the second searches them.
 * Per (step z, clip b, band of 16 rows) and source s it writes 8 int32, partial[(((z*B + b)*nband + band)*S + s)*8 + slot]:
 *   slot 0  n_f = |E(f_s)| in the band         slot 1  n_o = |E(y)| in the band
 *   slot 2  sum_q_fo    slot 4  sum_d2_fo    slot 6  max_d2_fo    over p in E(f_s), rows of the band, against all of E(y)
 *   slot 3  sum_q_of    slot 5  sum_d2_of    slot 7  max_d2_of    over p in E(y), rows of the band, against all of E(f_s)
 * A direction whose target set is empty has sum and max 0.  Over the bands slots 0-5 add and slots 6-7 are maximised (the
 * caller's, in int64: d2 <= 130050 and q <= 92321, so a band of <= 4096 queries stays below 2^31 and a frame need not).
 * No atomics, integers only: the same inputs give the same bits. */
int qt_edge_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels, const int* Ns,
                    const int32_t* const* n_devs, const float* y, int64_t y_clip_stride, int64_t y_step_stride,
                    const float* base1, int64_t base1_clip_stride, int64_t base1_step_stride, const float* base2,
                    int64_t base2_clip_stride, int64_t base2_step_stride, const uint8_t* pix_mask, float thr, int B, int n, int m,
                    uint64_t* planes, int32_t* partial, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QTMPNN_EDGES_H */
