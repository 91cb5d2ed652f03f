// Wide stream pool of the Seq2Seq model: the push of synthesize.WideSeq2SeqStreamPool -- up to 128 independent sessions (rows) on one Seq2Seq
// window decoder.  That model never reads an audio sample: a row's chunks only drive its clock.  So a tick travels without audio and the pool
// keeps no sample ring: the state is the word ring [B][W][3] with its counter n_words [B] and the sample counter written [B].
//   tg_wide_pool_push_words   the push of ONE packed device buffer: a header hdr [B][4] int32 = (n samples, 0, record count, record offset) per
//                             row -- tg_wide_pool_push's header; the second entry is not read -- and the rows' records concatenated.  Row b appends
//                             its records to its word ring and adds n to written[b]; a row with n == 0 and no records is skipped.  The header is
//                             the host's (it is validated before the upload); packed_row<false> (stream_rows.hpp) clamps the counts and the
//                             records' offset so that no index leaves the record slice.
// (tg_wide_pool_stage_text and tg_wide_pool_handover_smooth are stream_pool_seq.hip's kernels and launchers with the row limit ST_MAX_WIDE_ROWS:
// they live there.)
// One workgroup per row, plain loads and stores, no atomics, nothing waits on another workgroup; a row that is not selected leaves before any
// store and before any barrier.  The records go through the append every push body shares (stream_rows.hpp), so a row's word ring and counters
// after a tick are what tg_wide_pool_push leaves for the same header and records.
#include "stream_rows.hpp"

namespace tg {

constexpr int PW_THREADS = 256;         // a tick brings a handful of records per row: 3 m integers

__global__ __launch_bounds__(PW_THREADS) void wide_pool_push_words_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ recs,
                                                                          long recs_len, int m_max, int64_t* written, int32_t* __restrict__ word_ring,
                                                                          int64_t* n_words, int W) {
    const int b = blockIdx.x;
    const auto [n, off, m, roff] = packed_row<false>(hdr, b, 0, 0, m_max, recs_len);     // (no sample piece: the second entry is not loaded, off is 0)
    if (n == 0 && m == 0) return;                                     // (the whole workgroup, before any barrier: the row keeps its counters and ring)
    const long wr = written[b], cnt = n_words[b];
    __syncthreads();                                                  // every thread has the counters before thread 0 moves them
    word_ring_append_row<PW_THREADS>(b, (int)m, cnt, recs + 3 * roff, word_ring, W);
    if (threadIdx.x == 0) {
        written[b] = wr + n;
        n_words[b] = cnt + m;
    }
}

}  // namespace tg

using namespace tg;

extern "C" int tg_wide_pool_push_words(const int32_t* hdr, const int32_t* recs, int64_t recs_len, int32_t m_max, int32_t words_live, int64_t* written,
                                       int32_t* word_ring, int64_t* n_words, int32_t B, int32_t W, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_WIDE_ROWS && m_max >= 0 && W >= 1 && W <= ST_MAX_WORDS && words_live >= 0 && (int64_t)words_live + m_max <= W &&
                   recs_len >= m_max && recs_len <= (int64_t)B * m_max,
               "tg_wide_pool_push_words: outside the envelope 1 <= B <= %d, m_max >= 0, 1 <= W <= %d, words_live + m_max <= W -- the word ring would "
               "overwrite records a window still needs --, m_max <= recs_len <= B m_max (B=%d m_max=%d words_live=%d W=%d recs_len=%lld)",
               ST_MAX_WIDE_ROWS, ST_MAX_WORDS, B, m_max, words_live, W, (long long)recs_len);
    TG_REQUIRE(hdr && (recs || m_max == 0) && written && word_ring && n_words, "tg_wide_pool_push_words: null pointer");
    hipLaunchKernelGGL(wide_pool_push_words_kernel, dim3(B), dim3(PW_THREADS), 0, (hipStream_t)stream, hdr, recs, (long)recs_len, m_max, written,
                       word_ring, n_words, W);
    return check_launch("tg_wide_pool_push_words");
}
