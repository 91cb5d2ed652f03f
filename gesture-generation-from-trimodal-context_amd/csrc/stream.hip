// Streaming synthesis: the device side of synthesize.GestureStream -- audio and words arrive in pieces, windows are cut as they become complete.
//   tg_stream_push   appends a chunk [B][n] of samples to the per-row ring [B][R] at written[b] mod R (the chunk may straddle the wrap point) and
//                    the chunk's word records -- int32 triples (absolute window, frame in window, word id) -- to the per-row word ring [B][W][3]
//                    at n_words[b] mod W, then advances both counters.  One workgroup per row: it reads its row's counters, passes a barrier,
//                    copies, and its first thread writes the counters back, so nothing waits on another workgroup and nothing needs an atomic.
//   tg_stream_stage  cuts the inputs of window w = win[0] (device memory): audio_out[b][k] = ring[b][(w S + k) mod R] for k < min(A, written[b] - w S),
//                    zeros behind (the closing windows of a stream); text_out[b][f] = the id of the LAST pushed record with window w and frame f,
//                    else 0 (the reference's loop overwrites in word order, synthesize.py:112-116: the records are scanned oldest to newest by
//                    the one thread that owns the frame).
// Every counter lives in device memory: the launches are the same for every push and every window.  As in utterance.hip the device sees integers
// only -- the frame and the windows of a word are decided once by the host's Python doubles -- and samples move as bits: plain loads and stores.
#include "common.hpp"

namespace tg {

constexpr int ST_MAX_ROWS = 4;          // rows of a stream (the few-row decoders' lock-step limit)
constexpr int ST_MAX_WORDS = 1024;      // largest word ring per row: 12 KB of LDS in the stage kernel
constexpr int ST_MAX_FRAMES = 1024;     // frames of a window: one thread each
constexpr int ST_MAX_RING = 1 << 30;    // samples of a row's ring: positions and their sums stay inside an int
constexpr int ST_MAX_WINDOW = 1 << 25;  // samples of a window: the stage kernel's grid

__global__ __launch_bounds__(1024) void stream_push_kernel(const float* __restrict__ chunk, long chunk_stride, int n, const int32_t* __restrict__ recs,
                                                           int rec_stride, int m_max, float* __restrict__ ring, int64_t* __restrict__ written,
                                                           int32_t* __restrict__ word_ring, int64_t* __restrict__ n_words, int R, int W) {
    const int b = blockIdx.x;
    const long wr = written[b], cnt = n_words[b];
    int m = recs ? recs[(long)b * rec_stride] : 0;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
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

__global__ __launch_bounds__(256) void stream_stage_kernel(const float* __restrict__ ring, const int64_t* __restrict__ written,
                                                           const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                           const int32_t* __restrict__ win, int R, int S, int A, int W, int T,
                                                           float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    __shared__ int32_t rec[ST_MAX_WORDS * 3];
    const int b = blockIdx.x;
    const int w = win[0];
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

using namespace tg;

extern "C" int tg_stream_push(const float* chunk, int64_t chunk_stride, int32_t n, const int32_t* recs, int32_t rec_stride, int32_t m_max,
                              int32_t words_live, float* ring, int64_t* written, int32_t* word_ring, int64_t* n_words, int32_t B, int32_t R,
                              int32_t A, int32_t W, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_ROWS && n >= 1 && A >= 1 && W >= 1 && W <= ST_MAX_WORDS && (int64_t)R >= (int64_t)A + n && R <= ST_MAX_RING &&
                   chunk_stride >= n,
               "tg_stream_push: outside the envelope 1 <= B <= %d, n >= 1, A + n <= R <= 2^30, 1 <= W <= %d, chunk_stride >= n (B=%d n=%d R=%d A=%d "
               "W=%d chunk_stride=%lld)", ST_MAX_ROWS, ST_MAX_WORDS, B, n, R, A, W, (long long)chunk_stride);
    TG_REQUIRE(m_max >= 0 && words_live >= 0 && (int64_t)words_live + m_max <= W && (m_max == 0 || (recs && rec_stride >= 1 + 3 * (int64_t)m_max)),
               "tg_stream_push: outside the envelope words_live + m_max <= W -- the word ring would overwrite records a window still needs -- and "
               "rec_stride >= 1 + 3 m_max (words_live=%d m_max=%d W=%d rec_stride=%d)", words_live, m_max, W, rec_stride);
    TG_REQUIRE(chunk && ring && written && word_ring && n_words, "tg_stream_push: null pointer");
    hipLaunchKernelGGL(stream_push_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, chunk, (long)chunk_stride, n, m_max ? recs : nullptr, rec_stride,
                       m_max, ring, written, word_ring, n_words, R, W);
    return check_launch("tg_stream_push");
}

extern "C" int tg_stream_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                               int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio, int64_t* out_text, void* stream) {
    TG_REQUIRE(win && (out_audio || out_text), "tg_stream_stage: null pointer");
    TG_REQUIRE(!out_audio || (ring && written), "tg_stream_stage: audio output without the ring or its counter");
    TG_REQUIRE(!out_text || (word_ring && n_words), "tg_stream_stage: text output without the word ring or its counter");
    TG_REQUIRE(B >= 1 && B <= ST_MAX_ROWS && S >= 1 && A >= 1 && A <= ST_MAX_WINDOW && R > A && R <= ST_MAX_RING && W >= 1 && W <= ST_MAX_WORDS &&
                   T >= 1 && T <= ST_MAX_FRAMES,
               "tg_stream_stage: outside the envelope 1 <= B <= %d, S >= 1, 1 <= A <= 2^25, A + 1 <= R <= 2^30, 1 <= W <= %d, 1 <= T <= %d (B=%d R=%d S=%d "
               "A=%d W=%d T=%d)",
               ST_MAX_ROWS, ST_MAX_WORDS, ST_MAX_FRAMES, B, R, S, A, W, T);
    hipLaunchKernelGGL(stream_stage_kernel, dim3(B, out_audio ? cdiv(A, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, ring, written, word_ring,
                       n_words, win, R, S, A, W, T, out_audio, out_text);
    return check_launch("tg_stream_stage");
}
