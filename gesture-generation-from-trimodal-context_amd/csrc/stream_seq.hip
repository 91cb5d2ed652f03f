// Streaming synthesis of the Seq2Seq model: a window's word list from the word ring of csrc/stream.hip.
//   tg_stream_stage_text  reads the stream state tg_stream_push maintains -- word_ring [B][W][3] int32 triples (absolute window, frame in window,
//                         word id), the per-row counter n_words and the window index win[0], all in device memory -- and writes, for every
//                         row, out_text[b] = [SOS, the ids of EVERY record of window win[0] in push order, EOS, 0 ...] (Te int64 entries) and
//                         out_len[b] = count + 2: the unpadded list synthesize.seq2seq_window_text builds, padded with 0 = PAD, and its length.
//                         tg_stream_stage keeps only the last record of a frame; here two words on one frame are two list entries.
// One workgroup per row: the ring's live records are read oldest to newest, four per thread, flagged, and an integer prefix sum over the
// workgroup gives every kept record its place -- an order-preserving compaction without atomics; ids move as bits.  A row with more than
// Te - 2 records for the window is the host's to refuse before the push (it computes the records); the kernel clamps the count so that no
// index can leave the row.
#include "stream_rows.hpp"

namespace tg {

constexpr int SQ_MAX_TE = 128;          // longest list (the encoder's and the decoder's envelope)
constexpr int SQ_THREADS = ST_MAX_WORDS / 4;   // four records of the word ring per thread

__global__ __launch_bounds__(SQ_THREADS) void stream_stage_text_kernel(const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                                       const int32_t* __restrict__ win, int W, int Te, long long sos, long long eos,
                                                                       long long* __restrict__ out_text, long long* __restrict__ out_len) {
    __shared__ int s_scan[SQ_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int w = win[0];
    const long cnt = n_words[b];
    const long lo = cnt > W ? cnt - W : 0;                            // the ring holds the last W records, slot = index mod W
    const int live = cnt < 0 ? 0 : (int)(cnt - lo);
    const int s0 = (int)(lo % W);
    const int32_t* __restrict__ ring = word_ring + (long)b * W * 3;
    long long* __restrict__ row = out_text + (long)b * Te;
    int32_t id[4];
    bool hit[4];
    int c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * tid + q;                                    // age order: j = 0 is the oldest live record
        hit[q] = false;
        id[q] = 0;
        if (j < live) {
            int slot = s0 + j;                                        // live <= W: one subtraction wraps
            if (slot >= W) slot -= W;
            hit[q] = ring[3 * slot] == w;
            id[q] = ring[3 * slot + 2];
        }
        c += hit[q] ? 1 : 0;
    }
    s_scan[tid] = c;
    __syncthreads();
    for (int o = 1; o < SQ_THREADS; o <<= 1) {
        const int v = tid >= o ? s_scan[tid - o] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const int total = s_scan[SQ_THREADS - 1];
    const int kept = total < Te - 2 ? total : Te - 2;                 // (Te >= 2)
    int pos = s_scan[tid] - c;                                        // records kept in front of this thread's
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (hit[q]) {
            if (pos < kept) row[1 + pos] = (long long)id[q];
            ++pos;
        }
    if (tid == 0) {
        row[0] = sos;
        row[1 + kept] = eos;
        out_len[b] = kept + 2;
    }
    for (int p = kept + 2 + tid; p < Te; p += SQ_THREADS) row[p] = 0;
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
