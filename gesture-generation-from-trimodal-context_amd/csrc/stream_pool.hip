// Stream pool: the device side of synthesize.StreamPool -- up to four independent sessions (rows) on one window decoder, each with a clock of
// its own.  The state is stream.hip's (ring [B][R], written [B], word ring [B][W][3], n_words [B]) with a window counter PER ROW, win [B],
// and an int32 mask active [B] that says which rows a launch may touch.  A row that is not touched keeps every bit: no kernel here writes
// a counter, a ring slot or an output element of such a row.
//   tg_pool_push      tg_stream_push with a chunk length per row (by value: B <= 4); a row with n[b] == 0 and no records is skipped.
//   tg_pool_stage     tg_stream_stage for window win[b] of every row with active[b] != 0 (same copies, same "last record wins").
//   tg_pool_handover  the tail of a window in one launch, per active row: out = res, cross-faded with the row's tail where win[b] > 0
//                     (tg_window_blend's expression, operand for operand), tail = the last n_pre frames, the next window's seed
//                     (tg_make_pre_seq's layout [T][D + 1], or the plain [n_pre][D]), and -- behind a barrier -- win[b] += 1.
// tg_wide_pool_stage / tg_wide_pool_handover (synthesize.WideStreamPool, up to 128 rows) are the same two kernels behind the same checks.
// One workgroup (push, handover) or one grid column (stage) per row; nothing waits on another workgroup, nothing needs an atomic, and the
// results do not depend on the order in which the workgroups run.  The row bodies of push and stage are stream_rows.hpp's, shared with
// stream.hip (whose kernels serve every stream that shares a clock), and so are the bounds: here a row brings its own chunk length and
// window index, and a row that is idle leaves before the body.
#include "stream_rows.hpp"
#include "window_rows.hpp"

namespace tg {

struct PoolLens {
    int n[ST_MAX_ROWS];
};

__global__ __launch_bounds__(1024) void pool_push_kernel(const float* __restrict__ chunk, long chunk_stride, PoolLens lens,
                                                         const int32_t* __restrict__ recs, int rec_stride, int m_max, float* __restrict__ ring,
                                                         int64_t* __restrict__ written, int32_t* __restrict__ word_ring,
                                                         int64_t* __restrict__ n_words, int R, int W) {
    const int b = blockIdx.x;
    const int n = b == 0 ? lens.n[0] : (b == 1 ? lens.n[1] : (b == 2 ? lens.n[2] : lens.n[3]));
    int m = recs ? recs[(long)b * rec_stride] : 0;
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    if (n == 0 && m == 0) return;                                     // (the whole workgroup, before any barrier: the row keeps its counters and rings)
    const long wr = written[b], cnt = n_words[b];
    ring_push_row(b, n, m, wr, cnt, chunk, chunk_stride, recs, rec_stride, ring, written, word_ring, n_words, R, W);
}

__global__ __launch_bounds__(256) void pool_stage_kernel(const float* __restrict__ ring, const int64_t* __restrict__ written,
                                                         const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words,
                                                         const int32_t* __restrict__ win, const int32_t* __restrict__ active, int R, int S, int A,
                                                         int W, int T, float* __restrict__ out_audio, int64_t* __restrict__ out_text) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup, before any barrier)
    ring_stage_row(b, win[b], ring, written, word_ring, n_words, R, S, A, W, T, out_audio, out_text);
}

// seed_bit != 0: seed is pre_seq [B][T][D + 1]; else pre [B][n][D].  out and tail are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(256) void pool_handover_kernel(const float* __restrict__ res, float* out, float* tail, float* __restrict__ seed,
                                                            int seed_bit, int32_t* win, const int32_t* __restrict__ active, int T, int D, int n) {
    const int b = blockIdx.x;
    if (active[b] == 0) return;                                       // (the whole workgroup)
    const int w = win[b];
    // (window_rows.hpp: the row body, shared with the synthesis queue's hand-over)
    handover_row(res + (long)b * T * D, out + (long)b * T * D, tail + (long)b * n * D, seed + (long)b * (seed_bit ? T * (D + 1) : n * D), seed_bit, w > 0,
                 T, D, n);
    if (threadIdx.x == 0) win[b] = w + 1;                             // every thread read w before the barrier above
}

}  // namespace tg

using namespace tg;

extern "C" int tg_pool_push(const float* chunk, int64_t chunk_stride, int32_t n0, int32_t n1, int32_t n2, int32_t n3, const int32_t* recs,
                            int32_t rec_stride, int32_t m_max, int32_t words_live, float* ring, int64_t* written, int32_t* word_ring,
                            int64_t* n_words, int32_t B, int32_t R, int32_t A, int32_t W, void* stream) {
    PoolLens lens = {{n0, n1, n2, n3}};
    int64_t n_max = 0;
    bool rows_ok = B >= 1 && B <= ST_MAX_ROWS;
    for (int b = 0; b < ST_MAX_ROWS; ++b) {
        rows_ok = rows_ok && lens.n[b] >= 0 && (b < B || lens.n[b] == 0);
        n_max = lens.n[b] > n_max ? lens.n[b] : n_max;
    }
    TG_REQUIRE(rows_ok && (n_max >= 1 || m_max >= 1) && A >= 1 && W >= 1 && W <= ST_MAX_WORDS && (int64_t)R >= (int64_t)A + n_max && R > A &&
                   R <= ST_MAX_RING && chunk_stride >= n_max,
               "tg_pool_push: outside the envelope 1 <= B <= %d, n[b] >= 0 (0 for b >= B), a row with samples or records, A + max n <= R <= 2^30, "
               "A < R, 1 <= W <= %d, chunk_stride >= max n (B=%d n=%d,%d,%d,%d m_max=%d R=%d A=%d W=%d chunk_stride=%lld)",
               ST_MAX_ROWS, ST_MAX_WORDS, B, n0, n1, n2, n3, m_max, R, A, W, (long long)chunk_stride);
    TG_REQUIRE(m_max >= 0 && words_live >= 0 && (int64_t)words_live + m_max <= W && (m_max == 0 || (recs && rec_stride >= 1 + 3 * (int64_t)m_max)),
               "tg_pool_push: outside the envelope words_live + m_max <= W -- the word ring would overwrite records a window still needs -- and "
               "rec_stride >= 1 + 3 m_max (words_live=%d m_max=%d W=%d rec_stride=%d)", words_live, m_max, W, rec_stride);
    TG_REQUIRE((chunk || n_max == 0) && ring && written && word_ring && n_words, "tg_pool_push: null pointer");
    hipLaunchKernelGGL(pool_push_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, chunk, (long)chunk_stride, lens, m_max ? recs : nullptr, rec_stride,
                       m_max, ring, written, word_ring, n_words, R, W);
    return check_launch("tg_pool_push");
}

// The launchers of the stage and the hand-over: tg_pool_* (synthesize.StreamPool, rows <= ST_MAX_ROWS) and tg_wide_pool_* (WideStreamPool, rows <=
// ST_MAX_WIDE_ROWS) are the same kernels behind the same checks; an entry brings its name and its row limit.
static int launch_pool_stage(const char* who, int max_rows, const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words,
                             const int32_t* win, const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T,
                             float* out_audio, int64_t* out_text, void* stream) {
    TG_REQUIRE(win && active && (out_audio || out_text), "%s: null pointer", who);
    TG_REQUIRE(!out_audio || (ring && written), "%s: audio output without the ring or its counter", who);
    TG_REQUIRE(!out_text || (word_ring && n_words), "%s: text output without the word ring or its counter", who);
    TG_REQUIRE(B >= 1 && B <= max_rows && S >= 1 && A >= 1 && A <= ST_MAX_WINDOW && R > A && R <= ST_MAX_RING && W >= 1 && W <= ST_MAX_WORDS && T >= 1 &&
                   T <= ST_MAX_FRAMES,
               "%s: outside the envelope 1 <= B <= %d, S >= 1, 1 <= A <= 2^25, A + 1 <= R <= 2^30, 1 <= W <= %d, 1 <= T <= %d (B=%d R=%d S=%d A=%d W=%d "
               "T=%d)",
               who, max_rows, ST_MAX_WORDS, ST_MAX_FRAMES, B, R, S, A, W, T);
    hipLaunchKernelGGL(pool_stage_kernel, dim3(B, out_audio ? cdiv(A, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, ring, written, word_ring,
                       n_words, win, active, R, S, A, W, T, out_audio, out_text);
    return check_launch(who);
}

static int launch_pool_handover(const char* who, int max_rows, const float* res, float* out, float* tail, float* seed, int32_t seed_layout,
                                int32_t* win, const int32_t* active, int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    TG_REQUIRE(B >= 1 && B <= max_rows && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && T <= ST_MAX_FRAMES && n_pre < T &&
                   (seed_layout == 0 || seed_layout == 1),
               "%s: outside the envelope 1 <= B <= %d, 1 <= n_pre <= %d, 1 <= D <= %d, n_pre < T <= %d, seed_layout 0 (pre_seq [T][D + 1]) or 1 (pre "
               "[n_pre][D]) (B=%d n_pre=%d D=%d T=%d seed_layout=%d)",
               who, max_rows, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, B, n_pre, D, T, seed_layout);
    TG_REQUIRE(res && out && tail && seed && win && active, "%s: null pointer", who);
    hipLaunchKernelGGL(pool_handover_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, res, out, tail, seed, seed_layout == 0 ? 1 : 0, win, active, T,
                       D, n_pre);
    return check_launch(who);
}

#define POOL_STAGE_ARGS ring, written, word_ring, n_words, win, active, B, R, S, A, W, T, out_audio, out_text, stream
extern "C" int tg_pool_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                             const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio,
                             int64_t* out_text, void* stream) {
    return launch_pool_stage("tg_pool_stage", ST_MAX_ROWS, POOL_STAGE_ARGS);
}

extern "C" int tg_wide_pool_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                                  const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio,
                                  int64_t* out_text, void* stream) {
    return launch_pool_stage("tg_wide_pool_stage", ST_MAX_WIDE_ROWS, POOL_STAGE_ARGS);
}

#define POOL_HANDOVER_ARGS res, out, tail, seed, seed_layout, win, active, B, T, D, n_pre, stream
extern "C" int tg_pool_handover(const float* res, float* out, float* tail, float* seed, int32_t seed_layout, int32_t* win, const int32_t* active,
                                int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    return launch_pool_handover("tg_pool_handover", ST_MAX_ROWS, POOL_HANDOVER_ARGS);
}

extern "C" int tg_wide_pool_handover(const float* res, float* out, float* tail, float* seed, int32_t seed_layout, int32_t* win, const int32_t* active,
                                     int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    return launch_pool_handover("tg_wide_pool_handover", ST_MAX_WIDE_ROWS, POOL_HANDOVER_ARGS);
}
