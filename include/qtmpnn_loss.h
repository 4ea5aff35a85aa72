/*
 * qtmpnn_loss.h -- the weighted binary cross-entropy entries of libqtmpnn_hip.so, declared beside qtmpnn.h (whose conventions,
 * error codes and qt_last_error() it shares) the way qtmpnn_edges.h declares qt_edge_rollout: the tests of the project hold
 * qtmpnn.h and its binding table to a fixed list of 87 entry points, so entries added after them have their own header and their
 * own table (qtmpnn/_lib.py: _LOSS_SIGNATURES).
 */
#ifndef QTMPNN_LOSS_H
#define QTMPNN_LOSS_H

#include "qtmpnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The binary cross-entropy of qt_bce_rollout with the weights of qt_wsse_rollout and a weight on the positive class.  The
 * arguments are qt_wsse_rollout's / qt_wsse_rollout_bwd's (w (n*m) pixel weights and lam (nseg) step weights, fp32 device arrays,
 * non-negative; the caller forms the divisor) followed by pos_weight, passed by value, finite and > 0 (a captured graph keeps
 * the value it was captured with).  With o = outs[z][labels[p]*stride], L1 = max(log o, -100), L0 = max(log(1 - o), -100):
 *   partial[z][b*ntile + tile] = - sum over the tile's pixels with a node of lam[z] w[p] (pos_weight y L1 + (1 - y) L0)
 * and swys[z] (N_z, 2) receives per node [sum of w | sum of w*y] over the node's pixels.  qt_wbce_rollout_bwd writes
 *   gouts[z][i, 0] = g lam[z] (o_i sw_i - swy_i (pos_weight + o_i (1 - pos_weight))) / max(o_i (1 - o_i), 1e-12),
 * the per-pixel derivative (o - y (pos_weight + o (1 - pos_weight))) / (o (1 - o)) summed over the node with its weights (finite
 * at o = 0 and o = 1), zeros in columns 1..W-1, rows up to n_devs[z] where given.  Unit weights and pos_weight = 1 give
 * qt_bce_rollout's sums.  No atomics: the same bits on every run. */
int qt_wbce_rollout(int nseg, const float* const* outs, const int* out_strides, const int32_t* const* labels,
                    const uint8_t* const* levels, const int* Ns, float* const* swys, const float* y, int64_t y_clip_stride,
                    int64_t y_step_stride, const float* w, const float* lam, int B, int n, int m, float* partial,
                    float pos_weight, void* stream);
int qt_wbce_rollout_bwd(int nseg, const float* const* outs, const int* out_strides, const float* const* swys,
                        const int* Ns, const int32_t* const* n_devs, const float* g, const float* lam, int W,
                        float* const* gouts, float pos_weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QTMPNN_LOSS_H */
