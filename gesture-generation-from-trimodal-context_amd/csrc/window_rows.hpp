// The per-element and per-dimension bodies of a window's hand-over that more than one file runs: the cross-fade of a window's first n frames with
// the previous window's tail (stream_pool.hip, stream_pool_seq.hip; tg_window_blend's expression in losses.hip, operand for operand) and the
// least-squares segment of utterance.hip's smoothing (utterance.hip over the stacked windows, stream_pool_seq.hip on a window as it is handed
// over).  One body each, so that a window smoothed when it runs carries the bits the offline finish gives it.
#pragma once
#include "common.hpp"

namespace tg {

constexpr int PL_MAX_PRE = 8;           // tg_utterance_finish's n_pre and D
constexpr int PL_MAX_DIM = 64;

// frame j < n of a window that follows another: the tail's frame j fades out as the window's fades in
__device__ __forceinline__ float blend_head(float prev, float v, int j, int n) {
    return prev * (float)(n - j) / (float)(n + 1) + v * (float)(j + 1) / (float)(n + 1);
}

// y[0], y[D], ... y[(n - 1) D] <- P y: the fit of one dimension over n <= 3 PL_MAX_PRE frames as a projection (P: n x n fp64, row-major),
// accumulated in fp64 in the order k = 0 .. n - 1 and rounded once to fp32.  Multiply, then add, whatever the file's contraction setting is:
// numpy's doubles do not fuse.
__device__ __forceinline__ void project_segment(float* __restrict__ y, int D, int n, const double* __restrict__ P) {
#pragma clang fp contract(off)
    double v[3 * PL_MAX_PRE];
    for (int k = 0; k < n; ++k) v[k] = (double)y[(long)k * D];
    for (int r = 0; r < n; ++r) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += P[r * n + k] * v[k];
        y[(long)r * D] = (float)acc;
    }
}

}  // namespace tg
