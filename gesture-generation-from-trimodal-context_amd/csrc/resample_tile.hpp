// The resampler's tile body and its integer helpers (csrc/resample.hip has the definition of the conversion): what one workgroup does for up
// to TN outputs of one signal, shared by resample.hip (offline and streamed) and stream_preview.hip (the peek at a stream's flush).  One
// body, so that every caller gives an output the same K samples, the same K taps and the same order of fused multiply-adds.
#pragma once
#include "common.hpp"

namespace tg {

constexpr int RS_MAX_ROWS = 4;          // rows of a stream (stream_rows.hpp's ST_MAX_ROWS)
constexpr int RS_MAX_L = 640;           // phases (11 025 Hz: 640)
constexpr int RS_MAX_K = 512;           // taps per phase (192 kHz: 452)
constexpr int RS_THREADS = 256;
constexpr int RS_TAP_FLOATS = 8704;     // LDS for tap rows, stride K + 1: 16 rows of 513 fit, so a tile of 16 outputs always does
constexpr int RS_SPAN_FLOATS = 4096;    // LDS for a tile's input span: (TN - 1) M / L + 1 + K samples (255 * 12 + 1 + 512 at 192 kHz)

struct RsLens {
    int n[RS_MAX_ROWS];
};

// One output sample: K fused multiply-adds in increasing k from +0.  x: the K samples the output reads, t: its phase's taps.
__device__ __forceinline__ float resample_sample(const float* x, const float* t, int K) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(x[k], t[k], acc);
    return acc;
}

// Outputs [n0, n0 + cnt) of one signal by a whole workgroup of RS_THREADS threads, 1 <= cnt <= TN <= RS_THREADS (uniform over the workgroup).
// src(j): input sample j of the signal (absolute index, any int64), exact zero where the signal has none.  dst[r] receives output n0 + r.
// s_x / s_t: the workgroup's LDS (RS_SPAN_FLOATS / RS_TAP_FLOATS floats); the launcher chose TN so that both fit.  The tap rows are staged
// with stride K + 1 (odd: the lanes' rows start on different banks): all L phases if L <= TN, else row r = the phase of output n0 + r.
template <class Src>
__device__ __forceinline__ void resample_tile(long n0, int cnt, int L, int M, int K, int TN, const float* __restrict__ taps, Src src,
                                              float* __restrict__ dst, float* s_x, float* s_t) {
    const int tid = threadIdx.x, KP = K + 1;
    const long i_first = (n0 * M) / L;                                // i of the tile's first output; the span starts K/2 - 1 before it
    const long j0 = i_first - K / 2 + 1;
    const int span = (int)(((n0 + cnt - 1) * M) / L - i_first) + K;   // <= (TN - 1) M / L + 1 + K <= RS_SPAN_FLOATS
    for (int j = tid; j < span; j += RS_THREADS) s_x[j] = src(j0 + j);
    const bool all_phases = L <= TN;
    const int rows = all_phases ? L : cnt;
    for (int t = tid; t < rows * K; t += RS_THREADS) {
        const int r = t / K, k = t - r * K;
        const int p = all_phases ? r : (int)(((n0 + r) * M) % L);
        s_t[r * KP + k] = taps[p * K + k];
    }
    __syncthreads();
    if (tid < cnt) {
        const long nm = (n0 + tid) * M;
        const int off = (int)(nm / L - i_first), p = (int)(nm % L);
        dst[tid] = resample_sample(s_x + off, s_t + (all_phases ? p : tid) * KP, K);
    }
    __syncthreads();                                                  // the next tile of this workgroup stages into the same LDS
}

// ceil(n_in L / M): output samples of a signal of n_in samples
__device__ __host__ __forceinline__ long resampled_length(long n_in, int L, int M) { return n_in <= 0 ? 0 : (n_in * L + M - 1) / M; }
// outputs whose last tap, input sample i_n + K/2, is at or before sample p - 1: i_n <= p - 1 - K/2  <=>  n M < (p - K/2) L
__device__ __host__ __forceinline__ long resampled_ready(long p, int L, int M, int K) {
    const long q = p - K / 2;
    return q <= 0 ? 0 : (q * L - 1) / M + 1;
}

// outputs per tile: the largest power of two <= RS_THREADS whose tap rows and input span fit the LDS; 0 if none does
static int tile_outputs(int L, int M, int K) {
    for (int tn = RS_THREADS; tn >= 1; tn >>= 1) {
        const int64_t rows = L <= tn ? L : tn;
        if (rows * (K + 1) <= RS_TAP_FLOATS && (int64_t)(tn - 1) * M / L + 1 + K <= RS_SPAN_FLOATS) return tn;
    }
    return 0;
}

static bool geometry_ok(int L, int M, int K) { return L >= 1 && L <= RS_MAX_L && M >= 1 && K >= 2 && K <= RS_MAX_K && K % 2 == 0 && tile_outputs(L, M, K) >= 1; }

}  // namespace tg
