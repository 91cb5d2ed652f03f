// The per-element and per-dimension bodies of a window's hand-over that more than one file runs: the cross-fade of a window's first n frames with
// the previous window's tail (stream_pool.hip, stream_pool_seq.hip; tg_window_blend's expression in losses.hip, operand for operand) and the
// least-squares segment of utterance.hip's smoothing (utterance.hip over the stacked windows, stream_pool_seq.hip on a window as it is handed
// over).  One body each, so that a window smoothed when it runs carries the bits the offline finish gives it.
// And the row bodies the synthesis queue (queue.hip) shares with the kernels it is the counterpart of: a window's audio slice out of an
// utterance's plan (utterance.hip's tg_window_stage), the seed in tg_make_pre_seq's layout and a row's whole hand-over (stream_pool.hip's
// tg_pool_handover) -- the queue differs from them in WHERE a row reads and writes, never in what.
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

// One row of tg_window_stage's audio output, for a grid column of 256-thread workgroups with blockIdx.y = 0 .. cdiv(L, 1024): dst [L] = the
// slice [a0, a0 + nv) of the utterance src_base [len], clamped to its samples (the plan is the host's; the clamp keeps a wrong one inside the
// buffer), zeros behind.
__device__ __forceinline__ void stage_audio_row(const float* __restrict__ src_base, long len, long a0, long nv, float* __restrict__ dst, int L) {
    a0 = a0 < 0 ? 0 : (a0 > len ? len : a0);
    nv = nv < 0 ? 0 : (nv > len - a0 ? len - a0 : nv);
    if (nv > L) nv = L;
    const float* __restrict__ src = src_base + a0;
    // head: the elements before dst's first 16-byte boundary; body: 16-byte stores, 16-byte loads where src is aligned with dst and the four
    // samples are all valid; tail: what is left of the row
    const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2), L);
    if (blockIdx.y == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = (long)threadIdx.x < nv ? src[threadIdx.x] : 0.f;
    const int i = head + 4 * (int)(blockIdx.y * 256 + threadIdx.x);
    if (i + 3 < L) {
        f32x4 v;
        if (i + 3 < nv && (reinterpret_cast<uintptr_t>(src + i) & 15u) == 0) {
            v = *reinterpret_cast<const f32x4*>(src + i);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = i + q < nv ? src[i + q] : 0.f;
        }
        *reinterpret_cast<f32x4*>(dst + i) = v;
    } else {
        for (int q = i; q < L; ++q) dst[q] = q < nv ? src[q] : 0.f;
    }
}

// pre [T][D + 1] <- tg_make_pre_seq on a window whose first n frames are `frames` [n][D]: the frames with the constraint bit, zeros elsewhere
// (one 256-thread workgroup)
__device__ __forceinline__ void seed_pre_seq_row(float* __restrict__ pre, const float* frames, int T, int D, int n) {
    for (int i = threadIdx.x; i < T * (D + 1); i += 256) {
        const int c = i % (D + 1), t = i / (D + 1);
        pre[i] = t < n ? (c < D ? frames[t * D + c] : 1.f) : 0.f;
    }
}

// The tail of one row's window, by one 256-thread workgroup: o [T][D] = r, its first n frames cross-faded with the row's tail tl [n][D] where
// `follows` (tg_window_blend, with *p = v); then tl = o's last n frames and the next window's seed -- seed_bit != 0: pre_seq [T][D + 1], else
// pre [n][D].  o and tl are read and written here: no __restrict__ on them.  Every thread of the workgroup must call it (one barrier).
__device__ __forceinline__ void handover_row(const float* __restrict__ r, float* o, float* tl, float* __restrict__ seed, int seed_bit, bool follows,
                                             int T, int D, int n) {
    const int nD = n * D;
    for (int i = threadIdx.x; i < T * D; i += 256) {
        float v = r[i];
        if (follows && i < nD) v = blend_head(tl[i], v, i / D, n);
        o[i] = v;
    }
    __syncthreads();                                                  // the old tail has been read, the window is whole
    const float* last = o + (long)(T - n) * D;
    for (int i = threadIdx.x; i < nD; i += 256) tl[i] = last[i];
    if (seed_bit) {
        seed_pre_seq_row(seed, last, T, D, n);
    } else {
        for (int i = threadIdx.x; i < nD; i += 256) seed[i] = last[i];
    }
}

}  // namespace tg
