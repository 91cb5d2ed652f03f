// Streaming synthesis: the device side of synthesize.GestureStream -- audio and words arrive in pieces, windows are cut as they become complete.
//   tg_stream_push   appends a chunk [B][n] of samples to the per-row ring [B][R] at written[b] mod R (the chunk may straddle the wrap point) and
//                    the chunk's word records -- int32 triples (absolute window, frame in window, word id) -- to the per-row word ring [B][W][3]
//                    at n_words[b] mod W, then advances both counters.  One workgroup per row: it reads its row's counters, passes a barrier,
//                    copies, and its first thread writes the counters back, so nothing waits on another workgroup and nothing needs an atomic.
//   tg_stream_stage  cuts the inputs of window w = win[0] (device memory): the audio from the ring, zeros behind what was pushed, and per frame
//                    the id of the LAST pushed record of that window and frame (synthesize.py:112-116).
// Every counter lives in device memory: the launches are the same for every push and every window.  The row bodies are stream_rows.hpp's
// (stream_pool.hip runs the same ones on rows with clocks of their own): here every row has the chunk length n and the window win[0].
#include "stream_rows.hpp"

namespace tg {

__global__ __launch_bounds__(1024) void stream_push_kernel(const float* __restrict__ chunk, long chunk_stride, int n, const int32_t* __restrict__ recs,
                                                           int rec_stride, int m_max, float* __restrict__ ring, int64_t* __restrict__ written,
                                                           int32_t* __restrict__ word_ring, int64_t* __restrict__ n_words, int R, int W) {
    const int b = blockIdx.x;
    const long wr = written[b], cnt = n_words[b];
    int m = recs ? recs[(long)b * rec_stride] : 0;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    ring_push_row(b, n, m, wr, cnt, chunk, chunk_stride, recs, rec_stride, ring, written, word_ring, n_words, R, W);
}

__global__ __launch_bounds__(256) void stream_stage_kernel(const float* __restrict__ ring, const int64_t* __restrict__ written,
                                                           const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                           const int32_t* __restrict__ win, int R, int S, int A, int W, int T,
                                                           float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    ring_stage_row(blockIdx.x, win[0], ring, written, word_ring, n_words, R, S, A, W, T, out_audio, out_text);
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
