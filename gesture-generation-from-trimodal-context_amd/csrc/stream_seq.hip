// Streaming synthesis of the Seq2Seq model: a window's word list from the word ring of csrc/stream.hip.
//   tg_stream_stage_text  reads the stream state tg_stream_push maintains -- word_ring [B][W][3] int32 triples (absolute window, frame in window,
//                         word id), the per-row counter n_words and the window index win[0], all in device memory -- and writes, for every
//                         row, out_text[b] = [SOS, the ids of EVERY record of window win[0] in push order, EOS, 0 ...] (Te int64 entries) and
//                         out_len[b] = count + 2: the unpadded list synthesize.seq2seq_window_text builds, padded with 0 = PAD, and its length.
//                         tg_stream_stage keeps only the last record of a frame; here two words on one frame are two list entries.
// One workgroup per row; the row body -- an order-preserving compaction without atomics -- is stream_rows.hpp's ring_stage_text_row, shared with
// stream_pool_seq.hip (a window index per row).  A row with more than Te - 2 records for the window is the host's to refuse before the push
// (it computes the records); the body clamps the count so that no index can leave the row.
#include "stream_rows.hpp"

namespace tg {

__global__ __launch_bounds__(SQ_THREADS) void stream_stage_text_kernel(const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                                       const int32_t* __restrict__ win, int W, int Te, long long sos, long long eos,
                                                                       long long* __restrict__ out_text, long long* __restrict__ out_len) {
    ring_stage_text_row(blockIdx.x, win[0], word_ring, n_words, W, Te, sos, eos, out_text, out_len);
}

}  // namespace tg

using namespace tg;

extern "C" int tg_stream_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, int32_t B, int32_t W, int32_t Te,
                                    int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len, void* stream) {
    TG_REQUIRE(word_ring && n_words && win && out_text && out_len, "tg_stream_stage_text: null pointer");
    TG_REQUIRE(B >= 1 && B <= ST_MAX_ROWS && W >= 1 && W <= ST_MAX_WORDS && Te >= 2 && Te <= SQ_MAX_TE,
               "tg_stream_stage_text: outside the envelope 1 <= B <= %d, 1 <= W <= %d, 2 <= Te <= %d (B=%d W=%d Te=%d)", ST_MAX_ROWS, ST_MAX_WORDS,
               SQ_MAX_TE, B, W, Te);
    hipLaunchKernelGGL(stream_stage_text_kernel, dim3(B), dim3(SQ_THREADS), 0, (hipStream_t)stream, word_ring, n_words, win, W, Te, (long long)sos,
                       (long long)eos, (long long*)out_text, (long long*)out_len);
    return check_launch("tg_stream_stage_text");
}
