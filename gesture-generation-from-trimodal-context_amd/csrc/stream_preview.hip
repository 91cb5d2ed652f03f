// Stream preview: the device side of GestureStream.preview / StreamPool.preview -- the gestures of the window that is still filling, as the
// closing window of the utterance truncated now would give them, computed WITHOUT touching the stream: no kernel here stores to a ring, a
// counter, the tail, a seed, a window counter, the resampler's carry or the decoder's `out`.  What they write is scratch of the preview
// (extra, preview_out) and the decoder's text / audio inputs, which every real window rewrites before it reads them.
//   tg_resample_stream_peek  the flush branch of tg_resample_stream without its stores: per selected row the outputs from produced[b] up to
//                            ceil(consumed[b] L / M) out of [carry | zeros], into extra[b] -- resample_tile.hpp's tile body, the same chain.
//   tg_stream_stage_preview  tg_stream_stage / tg_pool_stage on a row that counts as written[b] + extra_n[b] samples long: the samples behind
//                            written[b] come from extra[b], zeros behind those (stream_rows.hpp's row body, EXTRA = true).  The window
//                            index is win[b], or one index by value (win == null) for rows that share a clock; the 1 to 4 extra_n by value.
//   tg_preview_handover      tg_pool_handover's first half and nothing else: preview_out[b] = res[b], its first n_pre frames cross-faded with
//                            tail[b] where the row's window index is > 0 (window_rows.hpp's blend_head: tg_window_blend's expression).
// One workgroup (or grid column) per row; a row that is not selected leaves before any store and before any barrier; nothing waits on another
// workgroup, no atomics, plain vector loads and stores.
#include "resample_tile.hpp"
#include "stream_rows.hpp"
#include "window_rows.hpp"

namespace tg {

struct PreviewLens {
    int n[ST_MAX_ROWS];
};

__global__ __launch_bounds__(RS_THREADS) void resample_peek_kernel(int row_mask, const float* __restrict__ taps, int L, int M, int K, int TN,
                                                                   const float* __restrict__ carry, const int64_t* __restrict__ consumed,
                                                                   const int64_t* __restrict__ produced, float* __restrict__ extra,
                                                                   long extra_stride) {
    __shared__ float s_x[RS_SPAN_FLOATS];
    __shared__ float s_t[RS_TAP_FLOATS];
    const int b = blockIdx.x;
    if (((row_mask >> b) & 1) == 0) return;                           // (the whole workgroup, before any barrier)
    const long c1 = consumed[b], o0 = produced[b];
    long n_new = resampled_length(c1, L, M) - o0;
    n_new = n_new < 0 ? 0 : (n_new > extra_stride ? extra_stride : n_new);     // (the host sized the row from the same integers)
    const float* __restrict__ cr = carry + (long)b * (K - 1);
    // tg_resample_stream's src with an empty chunk: the carry holds [c1 - (K - 1), c1), behind c1 the signal has ended
    auto src = [&](long j) -> float { return (j >= c1 || j < c1 - (K - 1)) ? 0.f : cr[j - c1 + (K - 1)]; };
    for (long t0 = 0; t0 < n_new; t0 += TN)
        resample_tile(o0 + t0, (int)(n_new - t0 < TN ? n_new - t0 : TN), L, M, K, TN, taps, src, extra + (long)b * extra_stride + t0, s_x, s_t);
}

__global__ __launch_bounds__(256) void stream_stage_preview_kernel(const float* __restrict__ ring, const int64_t* __restrict__ written,
                                                                   const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                                   const int32_t* __restrict__ win, int w_value,
                                                                   const int32_t* __restrict__ active, const float* __restrict__ extra,
                                                                   long extra_stride, PreviewLens lens, int R, int S, int A, int W, int T,
                                                                   float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    const int b = blockIdx.x;
    if (active && active[b] == 0) return;                             // (the whole workgroup, before any barrier)
    const int e = b == 0 ? lens.n[0] : (b == 1 ? lens.n[1] : (b == 2 ? lens.n[2] : lens.n[3]));
    ring_stage_row<true>(b, win ? win[b] : w_value, ring, written, word_ring, n_words, R, S, A, W, T, out_audio, out_text,
                         extra ? extra + (long)b * extra_stride : nullptr, e);      // (null only where every extra_n is 0)
}

__global__ __launch_bounds__(256) void preview_handover_kernel(const float* __restrict__ res, const float* __restrict__ tail,
                                                               const int32_t* __restrict__ win, int w_value, const int32_t* __restrict__ active,
                                                               int T, int D, int n, float* __restrict__ preview_out) {
    const int b = blockIdx.x;
    if (active && active[b] == 0) return;                             // (the whole workgroup)
    const int w = win ? win[b] : w_value;
    const float* __restrict__ r = res + (long)b * T * D;
    const float* __restrict__ tl = tail + (long)b * n * D;
    float* __restrict__ o = preview_out + (long)b * T * D;
    const int nD = n * D;
    for (int i = threadIdx.x; i < T * D; i += 256) {
        float v = r[i];
        if (w > 0 && i < nD) v = blend_head(tl[i], v, i / D, n);      // tg_window_blend (losses.hip), with *p = v
        o[i] = v;
    }
}

}  // namespace tg

using namespace tg;

extern "C" int tg_resample_stream_peek(int32_t row_mask, const float* taps, int32_t L, int32_t M, int32_t K, const float* carry,
                                       const int64_t* consumed, const int64_t* produced, float* extra, int64_t extra_stride, int32_t B,
                                       void* stream) {
    const bool rows_ok = B >= 1 && B <= RS_MAX_ROWS;
    TG_REQUIRE(rows_ok && row_mask >= 1 && row_mask < (1 << (rows_ok ? B : 1)) && geometry_ok(L, M, K),
               "tg_resample_stream_peek: outside the envelope 1 <= B <= %d, a row bit below 2^B, 1 <= L <= %d, M >= 1, K even in [2, %d] (B=%d "
               "row_mask=%d L=%d M=%d K=%d)", RS_MAX_ROWS, RS_MAX_L, RS_MAX_K, B, row_mask, L, M, K);
    // the most a flush adds: the outputs whose span reaches up to K/2 samples past the end (tg_resample_stream's bound with no chunk)
    const int64_t need = ((int64_t)(K / 2) * L + M - 1) / M + 1;
    TG_REQUIRE(extra_stride >= need, "tg_resample_stream_peek: outside the envelope extra_stride >= ceil((K/2) L / M) + 1 = %lld (extra_stride=%lld)",
               (long long)need, (long long)extra_stride);
    TG_REQUIRE(taps && carry && consumed && produced && extra, "tg_resample_stream_peek: null pointer");
    hipLaunchKernelGGL(resample_peek_kernel, dim3(B), dim3(RS_THREADS), 0, (hipStream_t)stream, row_mask, taps, L, M, K, tile_outputs(L, M, K), carry,
                       consumed, produced, extra, (long)extra_stride);
    return check_launch("tg_resample_stream_peek");
}

extern "C" int tg_stream_stage_preview(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words,
                                       const int32_t* win, int32_t w_value, const int32_t* active, const float* extra, int64_t extra_stride,
                                       int32_t e0, int32_t e1, int32_t e2, int32_t e3, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W,
                                       int32_t T, float* out_audio, int64_t* out_text, void* stream) {
    PreviewLens lens = {{e0, e1, e2, e3}};
    int64_t e_max = 0;
    bool rows_ok = B >= 1 && B <= ST_MAX_ROWS;
    for (int b = 0; b < ST_MAX_ROWS; ++b) {
        rows_ok = rows_ok && lens.n[b] >= 0 && (b < B || lens.n[b] == 0);
        e_max = lens.n[b] > e_max ? lens.n[b] : e_max;
    }
    TG_REQUIRE(out_audio || out_text, "tg_stream_stage_preview: null pointer");
    TG_REQUIRE(!out_audio || (ring && written), "tg_stream_stage_preview: audio output without the ring or its counter");
    TG_REQUIRE(!out_text || (word_ring && n_words), "tg_stream_stage_preview: text output without the word ring or its counter");
    TG_REQUIRE(rows_ok && S >= 1 && A >= 1 && A <= ST_MAX_WINDOW && R > A && R <= ST_MAX_RING && W >= 1 && W <= ST_MAX_WORDS && T >= 1 &&
                   T <= ST_MAX_FRAMES && extra_stride >= e_max && (e_max == 0 || (extra && out_audio)),
               "tg_stream_stage_preview: outside the envelope 1 <= B <= %d, S >= 1, 1 <= A <= 2^25, A + 1 <= R <= 2^30, 1 <= W <= %d, 1 <= T <= %d, "
               "extra_n[b] >= 0 (0 for b >= B), extra_stride >= max extra_n, extra and out_audio non-null with samples in it (B=%d R=%d S=%d A=%d "
               "W=%d T=%d extra_n=%d,%d,%d,%d extra_stride=%lld)",
               ST_MAX_ROWS, ST_MAX_WORDS, ST_MAX_FRAMES, B, R, S, A, W, T, e0, e1, e2, e3, (long long)extra_stride);
    hipLaunchKernelGGL(stream_stage_preview_kernel, dim3(B, out_audio ? cdiv(A, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, ring, written,
                       word_ring, n_words, win, w_value, active, extra, (long)extra_stride, lens, R, S, A, W, T, out_audio, out_text);
    return check_launch("tg_stream_stage_preview");
}

extern "C" int tg_preview_handover(const float* res, const float* tail, const int32_t* win, int32_t w_value, const int32_t* active, int32_t B,
                                   int32_t T, int32_t D, int32_t n_pre, float* preview_out, void* stream) {
    TG_REQUIRE(B >= 1 && B <= ST_MAX_ROWS && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && T <= ST_MAX_FRAMES && n_pre < T,
               "tg_preview_handover: outside the envelope 1 <= B <= %d, 1 <= n_pre <= %d, 1 <= D <= %d, n_pre < T <= %d (B=%d n_pre=%d D=%d T=%d)",
               ST_MAX_ROWS, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, B, n_pre, D, T);
    TG_REQUIRE(res && tail && preview_out, "tg_preview_handover: null pointer");
    hipLaunchKernelGGL(preview_handover_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, res, tail, win, w_value, active, T, D, n_pre, preview_out);
    return check_launch("tg_preview_handover");
}
