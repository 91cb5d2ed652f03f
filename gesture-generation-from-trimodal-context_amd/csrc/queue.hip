// Synthesis queue: the device side of synthesize.generate_gestures_queue -- N utterances on the R rows of one window decoder.  A row takes the
// next utterance the moment its own ends, on a schedule the host computed once as integers: sched [rounds][R][2] int32 = (utterance, window) of
// every row in every round, (-1, -1) where the row idles.  Each row counts its own rounds in device memory, rnd [R] int32: row b reads its
// entry sched[rnd[b]][b], so the host passes no round number and the two launches of a round are the same launches every round.
//   tg_queue_stage     tg_window_stage with the indirection row -> utterance: row b running (u, i) gets window i of utterance u out of the
//                      utterance batch's plan tables, the utterance's speaker id, the window's replayed draw, the Seq2Seq list with its length,
//                      and -- on the utterance's first window -- its seed in the row's seed buffer (both layouts of tg_pool_handover).
//   tg_queue_handover  tg_pool_handover with the window written into the utterance's rows of the stacked result instead of the decoder's out:
//                      total[u][i stride ..) = res[b] cross-faded with tail[b] where i > 0, tail[b], the next seed, and rnd[b] += 1.
// One workgroup (hand-over) or one grid column (stage) per row; plain loads and stores, no atomics, nothing waits on another workgroup, and a
// row that idles leaves before any store but the one to its own round counter.  Two rows never run the same utterance (the host checks the
// schedule before it uploads it), so no two workgroups write the same element.  The row bodies are window_rows.hpp's, shared with
// utterance.hip and stream_pool.hip: bits are theirs.  An entry that does not name a window of an utterance counts as idle.
#include "stream_rows.hpp"
#include "window_rows.hpp"

namespace tg {

constexpr int QU_MAX_ROWS = 128;
constexpr int QU_MAX_TEXT = 128;       // tg_stream_stage_text's Te
constexpr int QU_PLAN_COLS = 4;        // plan_win row (utterance.hip): audio_start, n_valid, spec_start, text length

// row b's entry of its own round: true and (u, i, g = the window's row in the plan tables) if it runs a window
__device__ __forceinline__ bool queue_entry(const int32_t* __restrict__ sched, const int32_t* rnd, int rounds, int R, int N,
                                            const int32_t* __restrict__ win_off, int b, int& u, int& i, long& g) {
    const int r = rnd[b];
    if (r < 0 || r >= rounds) return false;
    u = sched[((long)r * R + b) * 2 + 0];
    i = sched[((long)r * R + b) * 2 + 1];
    if (u < 0 || u >= N || i < 0) return false;
    const int w0 = win_off[u];
    if (i >= win_off[u + 1] - w0) return false;
    g = (long)w0 + i;
    return true;
}

// grid (R, cdiv(L, 1024) + 1 | 1) x 256.  Column 0 of a row also writes the row's text, length, speaker id, draw and -- first window -- seed.
__global__ __launch_bounds__(256) void queue_stage_kernel(const int32_t* __restrict__ sched, const int32_t* __restrict__ rnd, int rounds, int R, int N,
                                                          const float* __restrict__ audio, const int64_t* __restrict__ audio_off,
                                                          const int32_t* __restrict__ win_off, const int64_t* __restrict__ plan_win,
                                                          const int64_t* __restrict__ plan_text, int text_stride, int L, int text_w,
                                                          float* __restrict__ out_audio, int64_t* __restrict__ out_text, int64_t* __restrict__ out_len,
                                                          const int64_t* __restrict__ vids, int64_t* __restrict__ vid, const float* __restrict__ draws,
                                                          float* __restrict__ draw, int draw_w, const float* __restrict__ seeds,
                                                          const int32_t* __restrict__ seed_on, float* __restrict__ seed, int seed_bit, int T, int D,
                                                          int n) {
    const int b = blockIdx.x;
    int u, i;
    long g;
    if (!queue_entry(sched, rnd, rounds, R, N, win_off, b, u, i, g)) return;      // (the whole workgroup, before any store)
    if (blockIdx.y == 0) {
        if (out_text) {
            // the plan's row holds zeros behind the list (0 = PAD); a row narrower than the buffer is followed by zeros here
            int len = text_w < text_stride ? text_w : text_stride;
            if (out_len) {
                long ln = plan_win[g * QU_PLAN_COLS + 3];
                ln = ln < 2 ? 2 : (ln > len ? len : ln);
                len = (int)ln;
                if (threadIdx.x == 0) out_len[b] = ln;
            }
            for (int t = threadIdx.x; t < text_w; t += 256) out_text[(long)b * text_w + t] = t < len ? plan_text[g * text_stride + t] : 0;
        }
        if (vid && threadIdx.x == 0) vid[b] = vids[u];
        if (draw)
            for (int t = threadIdx.x; t < draw_w; t += 256) draw[(long)b * draw_w + t] = draws[g * draw_w + t];
        if (seed && i == 0) {
            const bool on = seeds && (!seed_on || seed_on[u] != 0);
            const float* __restrict__ s = on ? seeds + (long)u * n * D : nullptr;
            if (seed_bit) {
                float* __restrict__ pre = seed + (long)b * T * (D + 1);
                if (on) {
                    seed_pre_seq_row(pre, s, T, D, n);                                // WindowDecoder.seed(seed_seq): the frames and the constraint bit
                } else {
                    for (int k = threadIdx.x; k < T * (D + 1); k += 256) pre[k] = 0.f;     // WindowDecoder.seed(None)
                }
            } else {
                float* __restrict__ pre = seed + (long)b * n * D;
                for (int k = threadIdx.x; k < n * D; k += 256) pre[k] = on ? s[k] : 0.f;
            }
        }
    }
    if (!out_audio) return;
    stage_audio_row(audio + audio_off[u], audio_off[u + 1] - audio_off[u], plan_win[g * QU_PLAN_COLS + 0], plan_win[g * QU_PLAN_COLS + 1],
                    out_audio + (long)b * L, L);
}

// grid R x 256.  total and tail are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(256) void queue_handover_kernel(const float* __restrict__ res, float* total, long F, float* tail, float* __restrict__ seed,
                                                             int seed_bit, const int32_t* __restrict__ sched, int32_t* rnd, int rounds,
                                                             const int32_t* __restrict__ win_off, int R, int N, int T, int D, int n) {
    const int b = blockIdx.x;
    const int r = rnd[b];
    int u, i;
    long g;
    bool run = queue_entry(sched, rnd, rounds, R, N, win_off, b, u, i, g);
    const long f0 = run ? (long)i * (T - n) : 0;
    run = run && f0 + T <= F;                                         // (the host sized total for every window; this keeps a wrong F inside the buffer)
    if (run)                                                          // (uniform over the workgroup: handover_row holds a barrier)
        handover_row(res + (long)b * T * D, total + ((long)u * F + f0) * D, tail + (long)b * n * D, seed + (long)b * (seed_bit ? T * (D + 1) : n * D),
                     seed_bit, i > 0, T, D, n);
    if (threadIdx.x == 0 && r >= 0 && r < rounds) rnd[b] = r + 1;     // every thread read r first: nothing after a barrier reads rnd
}

}  // namespace tg

using namespace tg;

extern "C" int tg_queue_stage(const int32_t* sched, const int32_t* rnd, int32_t rounds, int32_t R, int32_t N, const float* audio, const int64_t* audio_off,
                              const int32_t* win_off, const int64_t* plan_win, const int64_t* plan_text, int32_t text_stride, int32_t L, int32_t text_w,
                              float* out_audio, int64_t* out_text, int64_t* out_len, const int64_t* vids, int64_t* vid, const float* draws, float* draw,
                              int32_t draw_w, const float* seeds, const int32_t* seed_on, float* seed, int32_t seed_layout, int32_t T, int32_t D,
                              int32_t n_pre, void* stream) {
    TG_REQUIRE(sched && rnd && win_off && plan_win && (out_audio || out_text), "tg_queue_stage: null pointer");
    TG_REQUIRE(rounds >= 1 && R >= 1 && R <= QU_MAX_ROWS && N >= 1 && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && n_pre < T &&
                   T <= ST_MAX_FRAMES && (seed_layout == 0 || seed_layout == 1),
               "tg_queue_stage: outside the envelope rounds >= 1, 1 <= R <= %d, N >= 1, 1 <= n_pre <= %d, 1 <= D <= %d, n_pre < T <= %d, seed_layout 0 "
               "(pre_seq [T][D + 1]) or 1 (pre [n_pre][D]) (rounds=%d R=%d N=%d n_pre=%d D=%d T=%d seed_layout=%d)",
               QU_MAX_ROWS, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, rounds, R, N, n_pre, D, T, seed_layout);
    TG_REQUIRE(!out_audio || (audio && audio_off && L > 0), "tg_queue_stage: audio output without audio, offsets or a length (L=%d)", L);
    TG_REQUIRE(!out_text || (plan_text && text_w > 0 && text_stride > 0), "tg_queue_stage: text output needs its table, text_w > 0 and text_stride > 0 (%d, %d)",
               text_w, text_stride);
    TG_REQUIRE(!out_len || (out_text && text_w >= 2 && text_w <= QU_MAX_TEXT),
               "tg_queue_stage: outside the envelope 2 <= Te <= %d for a text with lengths (Te=%d), or lengths without a text buffer", QU_MAX_TEXT, text_w);
    TG_REQUIRE(!vid == !vids, "tg_queue_stage: the speaker ids and the rows' buffer come together");
    TG_REQUIRE(!draw == !draws && (!draw || draw_w == 16 || draw_w == 32), "tg_queue_stage: replayed draws need their table, the rows' buffer and a width of 16 or 32 (draw_w=%d)",
               draw_w);
    TG_REQUIRE(seed || (!seeds && !seed_on), "tg_queue_stage: seeds without the rows' seed buffer");
    hipLaunchKernelGGL(queue_stage_kernel, dim3(R, out_audio ? cdiv(L, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, sched, rnd, rounds, R, N, audio,
                       audio_off, win_off, plan_win, plan_text, text_stride, L, text_w, out_audio, out_text, out_len, vids, vid, draws, draw, draw_w, seeds,
                       seed_on, seed, seed_layout == 0 ? 1 : 0, T, D, n_pre);
    return check_launch("tg_queue_stage");
}

extern "C" int tg_queue_handover(const float* res, float* total, int64_t F, float* tail, float* seed, int32_t seed_layout, const int32_t* sched, int32_t* rnd,
                                 int32_t rounds, const int32_t* win_off, int32_t R, int32_t N, int32_t T, int32_t D, int32_t n_pre, void* stream) {
    TG_REQUIRE(rounds >= 1 && R >= 1 && R <= QU_MAX_ROWS && N >= 1 && n_pre >= 1 && n_pre <= PL_MAX_PRE && D >= 1 && D <= PL_MAX_DIM && n_pre < T &&
                   T <= ST_MAX_FRAMES && F >= T && (seed_layout == 0 || seed_layout == 1),
               "tg_queue_handover: outside the envelope rounds >= 1, 1 <= R <= %d, N >= 1, 1 <= n_pre <= %d, 1 <= D <= %d, n_pre < T <= %d, F >= T, "
               "seed_layout 0 (pre_seq [T][D + 1]) or 1 (pre [n_pre][D]) (rounds=%d R=%d N=%d n_pre=%d D=%d T=%d F=%lld seed_layout=%d)",
               QU_MAX_ROWS, PL_MAX_PRE, PL_MAX_DIM, ST_MAX_FRAMES, rounds, R, N, n_pre, D, T, (long long)F, seed_layout);
    TG_REQUIRE(res && total && tail && seed && sched && rnd && win_off, "tg_queue_handover: null pointer");
    hipLaunchKernelGGL(queue_handover_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, res, total, (long)F, tail, seed, seed_layout == 0 ? 1 : 0, sched, rnd,
                       rounds, win_off, R, N, T, D, n_pre);
    return check_launch("tg_queue_handover");
}
