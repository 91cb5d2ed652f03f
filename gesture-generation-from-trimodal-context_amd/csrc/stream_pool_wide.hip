// Wide stream pool: the device side of synthesize.WideStreamPool -- stream_pool.hip's three launches for up to 128 independent sessions (rows)
// on one multimodal window decoder.  The state is stream_pool.hip's (ring [B][R], written [B], word ring [B][W][3], n_words [B], win [B],
// active [B]) and so are the row bodies (stream_rows.hpp, window_rows.hpp): what differs is that nothing per row is passed by value.
//   tg_wide_pool_push      the push of ONE packed device buffer: a header hdr [B][4] int32 = (n samples, sample offset, record count, record
//                          offset) per row, the rows' chunks concatenated without padding, the rows' records concatenated.  Row b appends
//                          samples[off .. off + n) and its records; a row with n == 0 and no records is skipped.  The header is the host's (it is
//                          validated before the upload); the kernel clamps every count and offset so that no index leaves the two slices.
//   tg_wide_pool_stage     tg_pool_stage's kernel body, B <= 128.
//   tg_wide_pool_handover  tg_pool_handover's kernel body, B <= 128.
// One workgroup (push, handover) or one grid column (stage) per row, plain loads and stores, no atomics, nothing waits on another workgroup; a row
// that is not selected leaves before any store and before any barrier: an idle row costs a workgroup that reads one or four integers and ends,
// so a launch over 128 rows of which one is busy takes the time of that one row.  For B <= 4 the entries write what the narrow ones write, bit for
// bit: the same bodies on the same operands.
#include "stream_rows.hpp"
#include "window_rows.hpp"

namespace tg {

__global__ __launch_bounds__(1024) void wide_pool_push_kernel(const int32_t* __restrict__ hdr, const float* __restrict__ samples, long samples_len,
                                                              const int32_t* __restrict__ recs, long recs_len, int n_max, int m_max,
                                                              float* __restrict__ ring, int64_t* __restrict__ written, int32_t* __restrict__ word_ring,
                                                              int64_t* __restrict__ n_words, int R, int W) {
    const int b = blockIdx.x;
    long n = hdr[4 * b], off = hdr[4 * b + 1], m = hdr[4 * b + 2], roff = hdr[4 * b + 3];
    // the slices [off, off + n) of samples [samples_len] and [roff, roff + m) of recs [recs_len][3]: inside them whatever the header says
    n = n < 0 ? 0 : (n > n_max ? n_max : n);
    off = off < 0 ? 0 : (off > samples_len ? samples_len : off);
    n = n > samples_len - off ? samples_len - off : n;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    roff = roff < 0 ? 0 : (roff > recs_len ? recs_len : roff);
    m = m > recs_len - roff ? recs_len - roff : m;
    if (n == 0 && m == 0) return;                                     // (the whole workgroup, before any barrier: the row keeps its counters and rings)
    const long wr = written[b], cnt = n_words[b];
    ring_push_row_from(b, (int)n, (int)m, wr, cnt, samples + off, recs + 3 * roff, ring, written, word_ring, n_words, R, W);
}

__global__ __launch_bounds__(256) void wide_pool_stage_kernel(const float* __restrict__ ring, const int64_t* __restrict__ written,
                                                              const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                              const int32_t* __restrict__ win, const int32_t* __restrict__ active, int R, int S, int A,
                                                              int W, int T, float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup, before any barrier)
    ring_stage_row(b, win[b], ring, written, word_ring, n_words, R, S, A, W, T, out_audio, out_text);
}

// seed_bit != 0: seed is pre_seq [B][T][D + 1]; else pre [B][n][D].  out and tail are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(256) void wide_pool_handover_kernel(const float* __restrict__ res, float* out, float* tail, float* __restrict__ seed,
                                                                 int seed_bit, int32_t* win, const int32_t* __restrict__ active, int T, int D, int n) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup)
    const int w = win[b];
    handover_row(res + (long)b * T * D, out + (long)b * T * D, tail + (long)b * n * D, seed + (long)b * (seed_bit ? T * (D + 1) : n * D), seed_bit, w > 0,
                 T, D, n);
    if (threadIdx.x == 0) win[b] = w + 1;                             // every thread read w before handover_row's barrier
}

}  // namespace tg

using namespace tg;

extern "C" int tg_wide_pool_push(const int32_t* hdr, const float* samples, int64_t samples_len, const int32_t* recs, int64_t recs_len, int32_t n_max,
                                 int32_t m_max, int32_t words_live, float* ring, int64_t* written, int32_t* word_ring, int64_t* n_words, int32_t B,
                                 int32_t R, int32_t A, int32_t W, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_WIDE_ROWS && n_max >= 0 && m_max >= 0 && (n_max >= 1 || m_max >= 1) && A >= 1 && W >= 1 && W <= ST_MAX_WORDS &&
                   (int64_t)R >= (int64_t)A + n_max && R > A && R <= ST_MAX_RING && samples_len >= n_max && samples_len <= (int64_t)B * n_max,
               "tg_wide_pool_push: outside the envelope 1 <= B <= %d, n_max >= 0, a row with samples or records, A + n_max <= R <= 2^30, A < R, "
               "1 <= W <= %d, n_max <= samples_len <= B n_max (B=%d n_max=%d m_max=%d R=%d A=%d W=%d samples_len=%lld)",
               ST_MAX_WIDE_ROWS, ST_MAX_WORDS, B, n_max, m_max, R, A, W, (long long)samples_len);
    TG_REQUIRE(words_live >= 0 && (int64_t)words_live + m_max <= W && recs_len >= m_max && recs_len <= (int64_t)B * m_max,
               "tg_wide_pool_push: outside the envelope words_live + m_max <= W -- the word ring would overwrite records a window still needs -- and "
               "m_max <= recs_len <= B m_max (words_live=%d m_max=%d W=%d recs_len=%lld)", words_live, m_max, W, (long long)recs_len);
    TG_REQUIRE(hdr && (samples || n_max == 0) && (recs || m_max == 0) && ring && written && word_ring && n_words, "tg_wide_pool_push: null pointer");
    hipLaunchKernelGGL(wide_pool_push_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, hdr, samples, (long)samples_len, recs, (long)recs_len, n_max,
                       m_max, ring, written, word_ring, n_words, R, W);
    return check_launch("tg_wide_pool_push");
}

extern "C" int tg_wide_pool_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                                  const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio,
                                  int64_t* out_text, void* stream) {
    TG_REQUIRE(win && active && (out_audio || out_text), "tg_wide_pool_stage: null pointer");
    TG_REQUIRE(!out_audio || (ring && written), "tg_wide_pool_stage: audio output without the ring or its counter");
    TG_REQUIRE(!out_text || (word_ring && n_words), "tg_wide_pool_stage: text output without the word ring or its counter");
    TG_REQUIRE(B >= 1 && B <= ST_MAX_WIDE_ROWS && S >= 1 && A >= 1 && A <= ST_MAX_WINDOW && R > A && R <= ST_MAX_RING && W >= 1 && W <= ST_MAX_WORDS &&
                   T >= 1 && T <= ST_MAX_FRAMES,
               "tg_wide_pool_stage: outside the envelope 1 <= B <= %d, S >= 1, 1 <= A <= 2^25, A + 1 <= R <= 2^30, 1 <= W <= %d, 1 <= T <= %d (B=%d R=%d "
               "S=%d A=%d W=%d T=%d)",
               ST_MAX_WIDE_ROWS, ST_MAX_WORDS, ST_MAX_FRAMES, B, R, S, A, W, T);
    hipLaunchKernelGGL(wide_pool_stage_kernel, dim3(B, out_audio ? cdiv(A, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, ring, written, word_ring,
                       n_words, win, active, R, S, A, W, T, out_audio, out_text);
    return check_launch("tg_wide_pool_stage");
}

extern "C" int tg_wide_pool_handover(const float* res, float* out, float* tail, float* seed, int32_t seed_layout, int32_t* win, const int32_t* active,
                                     int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_WIDE_ROWS && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && T <= ST_MAX_FRAMES && n_pre < T &&
                   (seed_layout == 0 || seed_layout == 1),
               "tg_wide_pool_handover: outside the envelope 1 <= B <= %d, 1 <= n_pre <= %d, 1 <= D <= %d, n_pre < T <= %d, seed_layout 0 (pre_seq "
               "[T][D + 1]) or 1 (pre [n_pre][D]) (B=%d n_pre=%d D=%d T=%d seed_layout=%d)",
               ST_MAX_WIDE_ROWS, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, B, n_pre, D, T, seed_layout);
    TG_REQUIRE(res && out && tail && seed && win && active, "tg_wide_pool_handover: null pointer");
    hipLaunchKernelGGL(wide_pool_handover_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, res, out, tail, seed, seed_layout == 0 ? 1 : 0, win,
                       active, T, D, n_pre);
    return check_launch("tg_wide_pool_handover");
}
