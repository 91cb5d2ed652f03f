// Wide stream pool: the push of synthesize.WideStreamPool -- up to 128 independent sessions (rows) on one multimodal window decoder.  The state
// is stream_pool.hip's (ring [B][R], written [B], word ring [B][W][3], n_words [B], win [B], active [B]) and so is the row body
// (stream_rows.hpp): what differs is that nothing per row is passed by value.
//   tg_wide_pool_push      the push of ONE packed device buffer: a header hdr [B][4] int32 = (n samples, sample offset, record count, record
//                          offset) per row, the rows' chunks concatenated without padding, the rows' records concatenated.  Row b appends
//                          samples[off .. off + n) and its records; a row with n == 0 and no records is skipped.  The header is the host's (it is
//                          validated before the upload); packed_row (stream_rows.hpp) clamps every count and offset so that no index leaves the two slices.
// (tg_wide_pool_stage and tg_wide_pool_handover are stream_pool.hip's kernels and launchers with the row limit ST_MAX_WIDE_ROWS: they live there.)
// One workgroup per row, plain loads and stores, no atomics, nothing waits on another workgroup; a row that is not selected leaves before any store
// and before any barrier: an idle row costs a workgroup that reads four integers and ends, so a launch over 128 rows of which one is busy takes
// the time of that one row.  For B <= 4 the entry writes what the narrow one writes, bit for bit: the same body on the same operands.
#include "stream_rows.hpp"

namespace tg {

__global__ __launch_bounds__(1024) void wide_pool_push_kernel(const int32_t* __restrict__ hdr, const float* __restrict__ samples, long samples_len,
                                                              const int32_t* __restrict__ recs, long recs_len, int n_max, int m_max,
                                                              float* __restrict__ ring, int64_t* __restrict__ written, int32_t* __restrict__ word_ring,
                                                              int64_t* __restrict__ n_words, int R, int W) {
    const int b = blockIdx.x;
    const auto [n, off, m, roff] = packed_row(hdr, b, n_max, samples_len, m_max, recs_len);
    if (n == 0 && m == 0) return;                                     // (the whole workgroup, before any barrier: the row keeps its counters and rings)
    const long wr = written[b], cnt = n_words[b];
    ring_push_row_from(b, (int)n, (int)m, wr, cnt, samples + off, recs + 3 * roff, ring, written, word_ring, n_words, R, W);
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
