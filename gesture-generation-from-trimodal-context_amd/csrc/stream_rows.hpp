// The row bodies of the stream kernels: what one row of the stream state -- sample ring [R], counter `written`, word ring [W][3], counter
// n_words -- does in a push and in the staging of a window.  stream.hip runs them for rows that share a clock (one chunk length, one window
// index), stream_pool.hip for rows with clocks of their own (a length and a window index per row, idle rows skipped); stream_seq.hip and
// stream_pool_seq.hip stage the Seq2Seq model's word list from the same word ring, in the same two ways.  The bounds are the files' bounds.
// stream_pool_wide.hip, stream_pool_wide_rs.hip and stream_pool_wide_seq.hip push rows whose lengths come from a packed header, which
// packed_row reads and clamps for all three.
// As in utterance.hip the device sees integers only and samples and ids move as bits: plain loads and stores.
#pragma once
#include "common.hpp"

namespace tg {

constexpr int ST_MAX_ROWS = 4;          // rows of a stream (the few-row decoders' lock-step limit)
constexpr int ST_MAX_WIDE_ROWS = 128;   // rows of a wide pool (stream_pool_wide.hip): the multimodal window decoder's and the queue's row limit
constexpr int ST_MAX_WORDS = 1024;      // largest word ring per row: 12 KB of LDS in the stage kernels
constexpr int ST_MAX_FRAMES = 1024;     // frames of a window: one thread each
constexpr int ST_MAX_RING = 1 << 30;    // samples of a row's ring: positions and their sums stay inside an int
constexpr int ST_MAX_WINDOW = 1 << 25;  // samples of a window: the stage kernels' grid

// Row b of a packed tick's header hdr [B][4] int32 = (n samples, sample offset, record count, record offset), clamped so that the slices
// [off, off + n) of samples [samples_len] and [roff, roff + m) of recs [recs_len][3] lie inside them whatever the header says.  SAMPLES = false
// (a tick without a sample piece, stream_pool_wide_seq.hip): n is a count that only has to be >= 0, and the second entry is not loaded.
struct PackedRow { long n, off, m, roff; };
template <bool SAMPLES = true>
__device__ __forceinline__ PackedRow packed_row(const int32_t* __restrict__ hdr, int b, int n_max, long samples_len, int m_max, long recs_len) {
    long n = hdr[4 * b], off = SAMPLES ? hdr[4 * b + 1] : 0, m = hdr[4 * b + 2], roff = hdr[4 * b + 3];
    n = n < 0 ? 0 : (SAMPLES && n > n_max ? n_max : n);
    if constexpr (SAMPLES) {
        off = off < 0 ? 0 : (off > samples_len ? samples_len : off);
        n = n > samples_len - off ? samples_len - off : n;
    }
    m = m < 0 ? 0 : (m > m_max ? m_max : m);
    roff = roff < 0 ? 0 : (roff > recs_len ? recs_len : roff);
    m = m > recs_len - roff ? recs_len - roff : m;
    return {n, off, m, roff};
}

// The records' half of a push, by a workgroup of THREADS threads: m records trip[0 .. 3 m) to row b's word ring at cnt mod W; it moves no counter.
// Every push body appends its records through it: ring_push_row_from below (1024 threads), stream_pool_wide_rs.hip (the resampler's workgroup, 256,
// whose samples do not come from a chunk) and stream_pool_wide_seq.hip (256, a push without samples).
template <int THREADS>
__device__ __forceinline__ void word_ring_append_row(int b, int m, long cnt, const int32_t* __restrict__ trip, int32_t* __restrict__ word_ring,
                                                     int W) {
    const int s0 = (int)(cnt % W);
    for (int t = threadIdx.x; t < 3 * m; t += THREADS) {
        int slot = s0 + t / 3;                                        // m <= W
        if (slot >= W) slot -= W;
        word_ring[((long)b * W + slot) * 3 + t % 3] = trip[t];
    }
}

// Row b of a push, by a workgroup of 1024 threads: n samples of chunk row b go to the ring at wr mod R (the chunk may straddle the wrap point),
// m records of recs row b (behind its count) to the word ring at cnt mod W, then thread 0 advances both counters.  wr = written[b] and
// cnt = n_words[b] were read by EVERY thread of the workgroup before it came here: the barrier below is what lets thread 0 move them.
// written and n_words are read (by the caller) and written (here): no __restrict__ on them.
// ring_push_row_from is the body: the row's samples are src[0 .. n) and its records' 3 m integers trip[0 .. 3 m), wherever the caller keeps them --
// a dense chunk and a table with a count per row (ring_push_row: stream.hip, stream_pool.hip) or slices of one packed buffer
// (stream_pool_wide.hip).
__device__ __forceinline__ void ring_push_row_from(int b, int n, int m, long wr, long cnt, const float* __restrict__ src,
                                                   const int32_t* __restrict__ trip, float* __restrict__ ring, int64_t* written,
                                                   int32_t* __restrict__ word_ring, int64_t* n_words, int R, int W) {
    __syncthreads();                                                  // every thread has the counters before thread 0 moves them
    const int p0 = (int)(wr % R);
    float* __restrict__ row = ring + (long)b * R;
    for (int k = threadIdx.x; k < n; k += 1024) {
        int p = p0 + k;                                               // n < R: one subtraction wraps
        if (p >= R) p -= R;
        row[p] = src[k];
    }
    word_ring_append_row<1024>(b, m, cnt, trip, word_ring, W);
    if (threadIdx.x == 0) {
        written[b] = wr + n;
        n_words[b] = cnt + m;
    }
}

__device__ __forceinline__ void ring_push_row(int b, int n, int m, long wr, long cnt, const float* __restrict__ chunk, long chunk_stride,
                                              const int32_t* __restrict__ recs, int rec_stride, float* __restrict__ ring, int64_t* written,
                                              int32_t* __restrict__ word_ring, int64_t* n_words, int R, int W) {
    ring_push_row_from(b, n, m, wr, cnt, chunk + (long)b * chunk_stride, recs ? recs + (long)b * rec_stride + 1 : nullptr, ring, written, word_ring,
                       n_words, R, W);
}

// Row b of the staging of window w, by the 256-thread workgroups (b, blockIdx.y) of a grid with cdiv(A, 1024) + 1 columns (one without audio):
// out_audio[b][k] = ring[b][(w S + k) mod R] for k < min(A, written[b] - w S), zeros behind (the closing windows of a stream);
// out_text[b][f] = the id of the LAST pushed record with window w and frame f, else 0 (the reference's loop overwrites in word order: the
// records are scanned oldest to newest by the one thread that owns the frame).  Either output may be null.  The whole workgroup comes here
// or none of it does: the text part has a barrier.
// EXTRA (stream_preview.hip): the row counts as written[b] + extra_n samples long, and the samples at positions written[b] <= p < written[b] +
// extra_n come from the side buffer extra_row[p - written[b]] -- what a push of them would have put into the ring, without the push.  The
// kernels that stage real windows instantiate EXTRA = false: for them nothing here changes.
template <bool EXTRA = false>
__device__ __forceinline__ void ring_stage_row(int b, int w, const float* __restrict__ ring, const int64_t* __restrict__ written,
                                               const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words, int R, int S, int A,
                                               int W, int T, float* __restrict__ out_audio, int64_t* __restrict__ out_text,
                                               const float* __restrict__ extra_row = nullptr, int extra_n = 0) {
    __shared__ int32_t rec[ST_MAX_WORDS * 3];
    if (out_text && blockIdx.y == 0) {
        const long cnt = n_words[b];
        const long lo = cnt > W ? cnt - W : 0;                        // the ring holds the last W records, slot = index mod W
        const int live = (int)(cnt - lo);
        for (int t = threadIdx.x; t < 3 * W; t += 256) rec[t] = word_ring[(long)b * W * 3 + t];
        __syncthreads();
        const int s0 = (int)(lo % W);
        for (int f = threadIdx.x; f < T; f += 256) {
            int32_t id = 0;
            int slot = s0;
            for (int j = 0; j < live; ++j) {                          // oldest to newest: the last match stays
                if (rec[3 * slot] == w && rec[3 * slot + 1] == f) id = rec[3 * slot + 2];
                if (++slot == W) slot = 0;
            }
            out_text[(long)b * T + f] = id;
        }
    }
    if (!out_audio) return;
    const long base = (long)w * S, wr = written[b];
    // samples [base + lost, base + nv) of the stream are in the ring; lost > 0 only if the host ran the window too late (older samples were
    // overwritten): those read as zeros, like everything from nv on
    const long gap = wr - base;                                       // EXTRA: window offsets from gap on are the side buffer's [0, extra_n)
    long nv = gap + (EXTRA ? extra_n : 0), lost = wr - R - base;
    nv = (nv < 0 || w < 0) ? 0 : (nv > A ? A : nv);                   // (a negative window index stages silence)
    lost = lost < 0 ? 0 : (lost > A ? A : lost);
    long nr = nv;                                                     // offsets below nr are in the ring (EXTRA = false: all of them)
    if (EXTRA) nr = gap < 0 ? 0 : (gap < nv ? gap : nv);
    const int p0 = (int)(base % R);
    const float* __restrict__ src = ring + (long)b * R;
    float* __restrict__ dst = out_audio + (long)b * A;
    auto at = [&](int k) -> float {                                   // A < R: one subtraction wraps
        if (k < lost || k >= nv) return 0.f;
        if (EXTRA && k >= nr) return extra_row[k - gap];              // 0 <= k - gap < extra_n: nr <= k < nv <= gap + extra_n
        int p = p0 + k;
        if (p >= R) p -= R;
        return src[p];
    };
    // head: the elements before dst's first 16-byte boundary; body: 16-byte stores, 16-byte loads where the four samples are valid, do not
    // straddle the wrap point and src is aligned with dst; tail: what is left of the row
    const int head = min((int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2), A);
    if (blockIdx.y == 0 && (int)threadIdx.x < head) dst[threadIdx.x] = at(threadIdx.x);
    const int i = head + 4 * (int)(blockIdx.y * 256 + threadIdx.x);
    if (i + 3 < A) {
        f32x4 v;
        int p = p0 + i;
        if (p >= R) p -= R;
        if (i >= lost && i + 3 < nr && p + 3 < R && (reinterpret_cast<uintptr_t>(src + p) & 15u) == 0) {
            v = *reinterpret_cast<const f32x4*>(src + p);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = at(i + q);
        }
        *reinterpret_cast<f32x4*>(dst + i) = v;
    } else {
        for (int q = i; q < A; ++q) dst[q] = at(q);
    }
}

constexpr int SQ_MAX_TE = 128;          // longest list (the encoder's and the decoder's envelope)
constexpr int SQ_THREADS = ST_MAX_WORDS / 4;   // four records of the word ring per thread

// Row b of the Seq2Seq model's text of window w, by a workgroup of SQ_THREADS threads: out_text[b] = [sos, the ids of EVERY record of window w
// in push order, eos, 0 ...] (Te entries), out_len[b] = count + 2.  The ring's live records are read oldest to newest, four per thread,
// flagged, and an integer prefix sum over the workgroup gives every kept record its place -- an order-preserving compaction without atomics;
// ids move as bits.  The count is clamped to Te - 2 so that no index can leave the row.  stream_seq.hip runs it for rows that share a window
// index, stream_pool_seq.hip with an index per row; the whole workgroup comes here or none of it does (barriers).
__device__ __forceinline__ void ring_stage_text_row(int b, int w, const int32_t* __restrict__ word_ring, const int64_t* __restrict__ n_words, int W,
                                                    int Te, long long sos, long long eos, long long* __restrict__ out_text,
                                                    long long* __restrict__ out_len) {
    __shared__ int s_scan[SQ_THREADS];
    const int tid = threadIdx.x;
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
