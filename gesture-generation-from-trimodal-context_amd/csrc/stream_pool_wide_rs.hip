// Wide stream pool at any sample rate: the push of synthesize.WideResampledStreamPool -- tg_wide_pool_push (stream_pool_wide.hip) with the
// stream resampler (resample.hip's resample_stream_kernel) in front of the ring, in ONE launch for up to 128 rows.
//   tg_wide_pool_push_resampled   the packed device buffer of tg_wide_pool_push, whose chunks now hold INPUT-rate samples.  Row b takes its n_b
//                                 samples into its resampler row (carry [K - 1], consumed, produced), computes the 16 kHz outputs that became
//                                 final -- or, for the ONE row flush_row whose input has ended, everything up to ceil(consumed L / M), zeros past
//                                 the end -- and stores output r into its sample ring at (written + r) mod R; then it rewrites the carry
//                                 behind a barrier, appends its records to the word ring and lets thread 0 store the four counters.
// The integers are resample_stream_kernel's (resampled_ready / resampled_length on the device's counters, mirrored on the host), the samples
// come from resample_tile and resample_sample, as they are: the same K samples, the same K taps, the same chain of fused multiply-adds as the
// offline and the streamed entry, so the ring holds the bits tg_resample_stream followed by tg_pool_push would have put there.  The tile body
// writes a contiguous tile, so a tile is staged in LDS and copied to the ring from there, each sample to its own position: a tile may straddle
// the ring's wrap point.
// One workgroup of RS_THREADS threads per row, plain loads and stores, no atomics, nothing waits on another workgroup; a row with no samples,
// no records and no flush leaves before any store and before any barrier.  The header is the host's; packed_row (stream_rows.hpp) clamps every
// count and offset, and the kernel the new output count to what the launcher checked the ring for, so that no index leaves a slice or a row.
// LDS: the tile body's two arrays (50 KB) and one tile of outputs (1 KB); three workgroups per CU fit.
#include "resample_tile.hpp"
#include "stream_rows.hpp"

namespace tg {

// carry, consumed, produced, written and n_words are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(RS_THREADS) void wide_pool_push_resampled_kernel(const int32_t* __restrict__ hdr, const float* __restrict__ samples,
                                                                              long samples_len, const int32_t* __restrict__ recs, long recs_len,
                                                                              int n_max, int m_max, int flush_row, const float* __restrict__ taps,
                                                                              int L, int M, int K, int TN, long out_max, float* carry,
                                                                              int64_t* consumed, int64_t* produced, float* __restrict__ ring,
                                                                              int64_t* written, int32_t* __restrict__ word_ring, int64_t* n_words,
                                                                              int R, int W) {
    __shared__ float s_x[RS_SPAN_FLOATS];
    __shared__ float s_t[RS_TAP_FLOATS];
    __shared__ float s_y[RS_THREADS];                                 // one tile of outputs (TN <= RS_THREADS)
    const int b = blockIdx.x, tid = threadIdx.x;
    const auto [n, off, m, roff] = packed_row(hdr, b, n_max, samples_len, m_max, recs_len);
    const bool flush = b == flush_row;
    if (n == 0 && m == 0 && !flush) return;                           // (the whole workgroup, before any barrier: the row keeps every bit)
    const bool resampling = n > 0 || flush;                           // a row with records only: its resampler row keeps every bit
    const long wr = written[b], cnt = n_words[b];
    long c0 = 0, o0 = 0, n_new = 0;
    if (resampling) {
        c0 = consumed[b];
        o0 = produced[b];
        n_new = (flush ? resampled_length(c0 + n, L, M) : resampled_ready(c0 + n, L, M, K)) - o0;
        n_new = n_new < 0 ? 0 : (n_new > out_max ? out_max : n_new);  // (the launcher checked R >= A + out_max: n_new < R, the window's samples stay)
    }
    const long c1 = c0 + n;
    const float* __restrict__ ch = samples + off;
    float* cr = carry + (long)b * (K - 1);
    // resample_stream_kernel's src: sample j of the row's signal from [carry | chunk]
    auto src = [&](long j) -> float {
        if (j >= c1 || j < c0 - (K - 1)) return 0.f;
        return j >= c0 ? ch[j - c0] : cr[j - c0 + (K - 1)];
    };
    float* __restrict__ row = ring + (long)b * R;
    const int p0 = (int)(wr % R);
    for (long t0 = 0; t0 < n_new; t0 += TN) {
        const int cnt_t = (int)(n_new - t0 < TN ? n_new - t0 : TN);
        resample_tile(o0 + t0, cnt_t, L, M, K, TN, taps, src, s_y, s_x, s_t);     // (ends behind a barrier: the tile is in s_y)
        if (tid < cnt_t) {
            int p = p0 + (int)t0 + tid;                               // p0 < R, t0 + tid < n_new < R <= 2^30: inside an int, one subtraction wraps
            if (p >= R) p -= R;
            row[p] = s_y[tid];
        }                                                             // (the next tile writes s_y behind resample_tile's first barrier)
    }
    float keep[2];                                                    // K - 1 <= 511 <= 2 RS_THREADS: the new carry, read before anyone writes it
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + q * RS_THREADS;
        keep[q] = resampling && i < K - 1 ? src(c1 - (K - 1) + i) : 0.f;     // a chunk shorter than K - 1 keeps the old carry's tail
    }
    __syncthreads();                                                  // every thread has the counters and its part of the old carry
    if (resampling) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + q * RS_THREADS;
            if (i < K - 1) cr[i] = keep[q];
        }
    }
    word_ring_append_row<RS_THREADS>(b, (int)m, cnt, recs + 3 * roff, word_ring, W);
    if (tid == 0) {
        if (resampling) {
            consumed[b] = c1;
            produced[b] = o0 + n_new;
        }
        written[b] = wr + n_new;
        n_words[b] = cnt + m;
    }
}

}  // namespace tg

using namespace tg;

extern "C" int tg_wide_pool_push_resampled(const int32_t* hdr, const float* samples, int64_t samples_len, const int32_t* recs, int64_t recs_len,
                                           int32_t n_max, int32_t m_max, int32_t words_live, int32_t flush_row, const float* taps, int32_t L,
                                           int32_t M, int32_t K, float* carry, int64_t* consumed, int64_t* produced, float* ring, int64_t* written,
                                           int32_t* word_ring, int64_t* n_words, int32_t B, int32_t R, int32_t A, int32_t W, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_WIDE_ROWS && flush_row >= -1 && flush_row < B && geometry_ok(L, M, K) && n_max >= 0 && m_max >= 0 &&
                   (n_max >= 1 || m_max >= 1 || flush_row >= 0) && A >= 1 && W >= 1 && W <= ST_MAX_WORDS,
               "tg_wide_pool_push_resampled: outside the envelope 1 <= B <= %d, -1 <= flush_row < B, 1 <= L <= %d, M >= 1, K even in [2, %d], a "
               "tile's span within %d samples, n_max >= 0, m_max >= 0, a row with samples, records or the flush, A >= 1, 1 <= W <= %d (B=%d "
               "flush_row=%d L=%d M=%d K=%d n_max=%d m_max=%d A=%d W=%d)",
               ST_MAX_WIDE_ROWS, RS_MAX_L, RS_MAX_K, RS_SPAN_FLOATS, ST_MAX_WORDS, B, flush_row, L, M, K, n_max, m_max, A, W);
    // the most a row can append: ceil(n L / M) outputs become final in a push, a flush adds those whose span reaches up to K/2 samples past the end
    const int64_t need = (((int64_t)n_max + (flush_row >= 0 ? K / 2 : 0)) * L + M - 1) / M + 1;
    TG_REQUIRE((int64_t)R >= (int64_t)A + need && R <= ST_MAX_RING && samples_len >= n_max && samples_len <= (int64_t)B * n_max,
               "tg_wide_pool_push_resampled: outside the envelope A + ceil((n_max + K/2 on a flush) L / M) + 1 = %lld <= R <= 2^30, n_max <= "
               "samples_len <= B n_max (R=%d A=%d n_max=%d samples_len=%lld)", (long long)(A + need), R, A, n_max, (long long)samples_len);
    TG_REQUIRE(words_live >= 0 && (int64_t)words_live + m_max <= W && recs_len >= m_max && recs_len <= (int64_t)B * m_max,
               "tg_wide_pool_push_resampled: outside the envelope words_live + m_max <= W -- the word ring would overwrite records a window still "
               "needs -- and m_max <= recs_len <= B m_max (words_live=%d m_max=%d W=%d recs_len=%lld)", words_live, m_max, W, (long long)recs_len);
    TG_REQUIRE(hdr && (samples || n_max == 0) && (recs || m_max == 0) && taps && carry && consumed && produced && ring && written && word_ring &&
                   n_words, "tg_wide_pool_push_resampled: null pointer");
    hipLaunchKernelGGL(wide_pool_push_resampled_kernel, dim3(B), dim3(RS_THREADS), 0, (hipStream_t)stream, hdr, samples, (long)samples_len, recs,
                       (long)recs_len, n_max, m_max, flush_row, taps, L, M, K, tile_outputs(L, M, K), (long)need, carry, consumed, produced, ring, written,
                       word_ring, n_words, R, W);
    return check_launch("tg_wide_pool_push_resampled");
}
