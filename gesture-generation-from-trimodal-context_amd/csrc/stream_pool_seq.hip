// Stream pool of the Seq2Seq model: the device side of synthesize.Seq2SeqStreamPool -- stream_pool.hip's state (a window counter win [B] per
// row, an int32 mask active [B]) under stream_seq.hip's text and the model's smoothing.
//   tg_pool_stage_text       tg_stream_stage_text for window win[b] of every row with active[b] != 0: out_text[b] = [SOS, every record of that
//                            window in push order, EOS, 0 ...], out_len[b] = count + 2 (the same row body, stream_rows.hpp).
//   tg_pool_handover_smooth  tg_pool_handover for the plain seed [n_pre][D], plus the smoothing of the window that is handed over: per active
//                            row out = res, cross-faded with the row's tail where win[b] > 0; behind a barrier frames [0, 3 n_pre) of out are
//                            replaced by their cubic least-squares fit (utterance.hip's projection, window_rows.hpp: the bits of
//                            tg_utterance_finish(smooth) on that window); tail = frames [T - n_pre, T), seed = tail, win[b] += 1.
// Why the fit may run here: with 3 n_pre <= T - n_pre window i's segment lies inside the window's own first T - n_pre frames, its values before
// the fit are final once the window has been cross-faded, and the next window's seed and cross-fade take frames [T - n_pre, T), which no
// segment touches -- so the tail and the seed are copied from frames the fit does not write, and no second barrier is needed.
// One workgroup per row, no atomics, nothing waits on another workgroup and the results do not depend on the order in which the workgroups
// run.  A row with active[b] == 0 leaves before any barrier: no text, length, output, tail, seed or counter of it is written.
// tg_wide_pool_stage_text / tg_wide_pool_handover_smooth (synthesize.WideSeq2SeqStreamPool, up to 128 rows) are the same two kernels behind the
// same checks; that pool's push is stream_pool_wide_seq.hip.
#include "stream_rows.hpp"
#include "window_rows.hpp"

namespace tg {

__global__ __launch_bounds__(SQ_THREADS) void pool_stage_text_kernel(const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                                     const int32_t* __restrict__ win, const int32_t* __restrict__ active, int W,
                                                                     int Te, long long sos, long long eos, long long* __restrict__ out_text,
                                                                     long long* __restrict__ out_len) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup, before any barrier)
    ring_stage_text_row(b, win[b], word_ring, n_words, W, Te, sos, eos, out_text, out_len);
}

// out and tail are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(256) void pool_handover_smooth_kernel(const float* __restrict__ res, float* out, float* tail, float* __restrict__ seed,
                                                                   int32_t* win, const int32_t* __restrict__ active,
                                                                   const double* __restrict__ proj, int T, int D, int n) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup)
    const int w = win[b];
    const float* __restrict__ r = res + (long)b * T * D;
    float* o = out + (long)b * T * D;
    float* tl = tail + (long)b * n * D;
    const int nD = n * D;
    for (int i = threadIdx.x; i < T * D; i += 256) {
        float v = r[i];
        if (w > 0 && i < nD) v = blend_head(tl[i], v, i / D, n);
        o[i] = v;
    }
    __syncthreads();                                                  // the old tail has been read, the window is whole
    if ((int)threadIdx.x < D) project_segment(o + threadIdx.x, D, 3 * n, proj);      // frames [0, 3 n): one thread per dimension
    const float* last = o + (long)(T - n) * D;                        // frames [T - n, T), 3 n <= T - n: not the segment's
    float* __restrict__ pre = seed + (long)b * nD;
    for (int i = threadIdx.x; i < nD; i += 256) {
        const float v = last[i];
        tl[i] = v;
        pre[i] = v;
    }
    if (threadIdx.x == 0) win[b] = w + 1;                             // every thread read w before the barrier above
}

}  // namespace tg

using namespace tg;

// The launchers: tg_pool_* (synthesize.Seq2SeqStreamPool, rows <= ST_MAX_ROWS) and tg_wide_pool_* (WideSeq2SeqStreamPool, rows <= ST_MAX_WIDE_ROWS)
// are the same kernels behind the same checks; an entry brings its name and its row limit (as stream_pool.hip's do).
static int launch_pool_stage_text(const char* who, int max_rows, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                                  const int32_t* active, int32_t B, int32_t W, int32_t Te, int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len,
                                  void* stream) {
    TG_REQUIRE(word_ring && n_words && win && active && out_text && out_len, "%s: null pointer", who);
    TG_REQUIRE(B >= 1 && B <= max_rows && W >= 1 && W <= ST_MAX_WORDS && Te >= 2 && Te <= SQ_MAX_TE,
               "%s: outside the envelope 1 <= B <= %d, 1 <= W <= %d, 2 <= Te <= %d (B=%d W=%d Te=%d)", who, max_rows, ST_MAX_WORDS, SQ_MAX_TE, B, W, Te);
    hipLaunchKernelGGL(pool_stage_text_kernel, dim3(B), dim3(SQ_THREADS), 0, (hipStream_t)stream, word_ring, n_words, win, active, W, Te,
                       (long long)sos, (long long)eos, (long long*)out_text, (long long*)out_len);
    return check_launch(who);
}

static int launch_pool_handover_smooth(const char* who, int max_rows, const float* res, float* out, float* tail, float* seed, int32_t* win,
                                       const int32_t* active, const double* proj, int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    TG_REQUIRE(B >= 1 && B <= max_rows && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && T <= ST_MAX_FRAMES &&
                   (int64_t)3 * n_pre <= (int64_t)T - n_pre,
               "%s: outside the envelope 1 <= B <= %d, 1 <= n_pre <= %d, 1 <= D <= %d, 3 n_pre <= T - n_pre (the smoothing "
               "segment inside the window's first T - n_pre frames), T <= %d (B=%d n_pre=%d D=%d T=%d)",
               who, max_rows, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, B, n_pre, D, T);
    TG_REQUIRE(res && out && tail && seed && win && active && proj, "%s: null pointer", who);
    hipLaunchKernelGGL(pool_handover_smooth_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, res, out, tail, seed, win, active, proj, T, D, n_pre);
    return check_launch(who);
}

#define POOL_STAGE_TEXT_ARGS word_ring, n_words, win, active, B, W, Te, sos, eos, out_text, out_len, stream
extern "C" int tg_pool_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, const int32_t* active, int32_t B, int32_t W,
                                  int32_t Te, int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len, void* stream) {
    return launch_pool_stage_text("tg_pool_stage_text", ST_MAX_ROWS, POOL_STAGE_TEXT_ARGS);
}

extern "C" int tg_wide_pool_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, const int32_t* active, int32_t B,
                                       int32_t W, int32_t Te, int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len, void* stream) {
    return launch_pool_stage_text("tg_wide_pool_stage_text", ST_MAX_WIDE_ROWS, POOL_STAGE_TEXT_ARGS);
}

#define POOL_HANDOVER_SMOOTH_ARGS res, out, tail, seed, win, active, proj, B, T, D, n_pre, stream
extern "C" int tg_pool_handover_smooth(const float* res, float* out, float* tail, float* seed, int32_t* win, const int32_t* active, const double* proj,
                                       int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    return launch_pool_handover_smooth("tg_pool_handover_smooth", ST_MAX_ROWS, POOL_HANDOVER_SMOOTH_ARGS);
}

extern "C" int tg_wide_pool_handover_smooth(const float* res, float* out, float* tail, float* seed, int32_t* win, const int32_t* active,
                                            const double* proj, int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    return launch_pool_handover_smooth("tg_wide_pool_handover_smooth", ST_MAX_WIDE_ROWS, POOL_HANDOVER_SMOOTH_ARGS);
}
