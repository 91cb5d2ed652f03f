// The row bodies of the stream kernels: what one row of the stream state -- sample ring [R], counter `written`, word ring [W][3], counter
// n_words -- does in a push and in the staging of a window.  stream.hip runs them for rows that share a clock (one chunk length, one window
// index), stream_pool.hip for rows with clocks of their own (a length and a window index per row, idle rows skipped); stream_seq.hip reads the
// same word ring.  The bounds are the three files' bounds.
// As in utterance.hip the device sees integers only and samples and ids move as bits: plain loads and stores.
#pragma once
#include "common.hpp"

namespace tg {

constexpr int ST_MAX_ROWS = 4;          // rows of a stream (the few-row decoders' lock-step limit)
constexpr int ST_MAX_WORDS = 1024;      // largest word ring per row: 12 KB of LDS in the stage kernels
constexpr int ST_MAX_FRAMES = 1024;     // frames of a window: one thread each
constexpr int ST_MAX_RING = 1 << 30;    // samples of a row's ring: positions and their sums stay inside an int
constexpr int ST_MAX_WINDOW = 1 << 25;  // samples of a window: the stage kernels' grid

// Row b of a push, by a workgroup of 1024 threads: n samples of chunk row b go to the ring at wr mod R (the chunk may straddle the wrap point),
// m records of recs row b (behind its count) to the word ring at cnt mod W, then thread 0 advances both counters.  wr = written[b] and
// cnt = n_words[b] were read by EVERY thread of the workgroup before it came here: the barrier below is what lets thread 0 move them.
// written and n_words are read (by the caller) and written (here): no __restrict__ on them.
__device__ __forceinline__ void ring_push_row(int b, int n, int m, long wr, long cnt, const float* __restrict__ chunk, long chunk_stride,
                                              const int32_t* __restrict__ recs, int rec_stride, float* __restrict__ ring, int64_t* written,
                                              int32_t* __restrict__ word_ring, int64_t* n_words, int R, int W) {
    __syncthreads();                                                  // every thread has the counters before thread 0 moves them
    const int p0 = (int)(wr % R);
    float* __restrict__ row = ring + (long)b * R;
    const float* __restrict__ src = chunk + (long)b * chunk_stride;
    for (int k = threadIdx.x; k < n; k += 1024) {
        int p = p0 + k;                                               // n < R: one subtraction wraps
        if (p >= R) p -= R;
        row[p] = src[k];
    }
    const int s0 = (int)(cnt % W);
    for (int t = threadIdx.x; t < 3 * m; t += 1024) {
        int slot = s0 + t / 3;                                        // m <= W
        if (slot >= W) slot -= W;
        word_ring[((long)b * W + slot) * 3 + t % 3] = recs[(long)b * rec_stride + 1 + t];
    }
    if (threadIdx.x == 0) {
        written[b] = wr + n;
        n_words[b] = cnt + m;
    }
}

// Row b of the staging of window w, by the 256-thread workgroups (b, blockIdx.y) of a grid with cdiv(A, 1024) + 1 columns (one without audio):
// out_audio[b][k] = ring[b][(w S + k) mod R] for k < min(A, written[b] - w S), zeros behind (the closing windows of a stream);
// out_text[b][f] = the id of the LAST pushed record with window w and frame f, else 0 (the reference's loop overwrites in word order: the
// records are scanned oldest to newest by the one thread that owns the frame).  Either output may be null.  The whole workgroup comes here
// or none of it does: the text part has a barrier.
__device__ __forceinline__ void ring_stage_row(int b, int w, const float* __restrict__ ring, const int64_t* __restrict__ written,
                                               const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words, int R, int S, int A,
                                               int W, int T, float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    __shared__ int32_t rec[ST_MAX_WORDS * 3];
    if (out_text && blockIdx.y == 0) {
        const long cnt = n_words[b];
        const long lo = cnt > W ? cnt - W : 0;                        // the ring holds the last W records, slot = index mod W
        const int live = (int)(cnt - lo);
        for (int t = threadIdx.x; t < 3 * W; t += 256) rec[t] = word_ring[(long)b * W * 3 + t];
        __syncthreads();
        const int s0 = (int)(lo % W);
        for (int f = threadIdx.x; f < T; f += 256) {
            int32_t id = 0;
            int slot = s0;
            for (int j = 0; j < live; ++j) {                          // oldest to newest: the last match stays
                if (rec[3 * slot] == w && rec[3 * slot + 1] == f) id = rec[3 * slot + 2];
                if (++slot == W) slot = 0;
            }
            out_text[(long)b * T + f] = id;
        }
    }
    if (!out_audio) return;
    const long base = (long)w * S, wr = written[b];
    // samples [base + lost, base + nv) of the stream are in the ring; lost > 0 only if the host ran the window too late (older samples were
    // overwritten): those read as zeros, like everything from nv on
    long nv = wr - base, lost = wr - R - base;
    nv = (nv < 0 || w < 0) ? 0 : (nv > A ? A : nv);                   // (a negative window index stages silence)
    lost = lost < 0 ? 0 : (lost > A ? A : lost);
    const int p0 = (int)(base % R);
    const float* __restrict__ src = ring + (long)b * R;
    float* __restrict__ dst = out_audio + (long)b * A;
    auto at = [&](int k) -> float {                                   // A < R: one subtraction wraps
        if (k < lost || k >= nv) return 0.f;
        int p = p0 + k;
        if (p >= R) p -= R;
        return src[p];
    };
    // head: the elements before dst's first 16-byte boundary; body: 16-byte stores, 16-byte loads where the four samples are valid, do not
    // straddle the wrap point and src is aligned with dst; tail: what is left of the row
    const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2), A);
    if (blockIdx.y == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = at(threadIdx.x);
    const int i = head + 4 * (int)(blockIdx.y * 256 + threadIdx.x);
    if (i + 3 < A) {
        f32x4 v;
        int p = p0 + i;
        if (p >= R) p -= R;
        if (i >= lost && i + 3 < nv && p + 3 < R && (reinterpret_cast<uintptr_t>(src + p) & 15u) == 0) {
            v = *reinterpret_cast<const f32x4*>(src + p);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = at(i + q);
        }
        *reinterpret_cast<f32x4*>(dst + i) = v;
    } else {
        for (int q = i; q < A; ++q) dst[q] = at(q);
    }
}

}  // namespace tg
