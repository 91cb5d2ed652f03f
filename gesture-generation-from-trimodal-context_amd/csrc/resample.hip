// Sample-rate conversion to 16 kHz on the device: rational polyphase resampling by L / M (L = 16000 / g, M = input_sr / g, g their gcd) with a
// host-made tap table [L][K] fp32 (resample.py: Kaiser-windowed sinc, K taps per phase, K even).  Output sample n sits at input position
// n M / L: i_n = (n M) div L, phase p_n = (n M) mod L, and
//     y[n] = sum_{k = 0 .. K-1} x[i_n - K/2 + 1 + k] * tap[p_n][k],         samples outside the signal are exact zeros,
// accumulated in fp32 in increasing k as ONE chain of fused multiply-adds (resample_sample).
//   tg_resample         offline and ragged: B signals packed in one buffer (int64 offsets in and out, device memory), grid (tile, row).
//   tg_resample_stream  1 to 4 rows whose input arrives in chunks (lengths by value, like tg_pool_push).  Per row, in device memory: the last
//                       K - 1 input samples (carry), the count of input samples consumed and the count of output samples produced.  A push
//                       computes the outputs whose whole tap span has arrived (or, with the row's flush bit, everything up to
//                       ceil(consumed L / M), zeros past the end), rewrites the carry behind a barrier and lets thread 0 store the counters.
//                       A row with no samples and no flush bit leaves before any store and keeps every bit.
// Both kernels run the same tile body (resample_tile) and the same sample body: the tile's input span -- zeros where the signal has none --
// and the tap rows its outputs use are staged in LDS, then one thread per output runs the chain.  A streamed signal therefore gives the bits
// of the offline call: each output sees the same K samples, the same K taps and the same order.  Integers decide everything else.
// One workgroup per (tile, row) or per row; nothing waits on another workgroup, no atomics.  Plain vector loads and stores only.
#include "resample_tile.hpp"

namespace tg {

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const int64_t* __restrict__ in_off,
                                                              const int64_t* __restrict__ out_off, const float* __restrict__ taps, int L, int M,
                                                              int K, int TN, float* __restrict__ y) {
    __shared__ float s_x[RS_SPAN_FLOATS];
    __shared__ float s_t[RS_TAP_FLOATS];
    const int b = blockIdx.y;
    const long x0 = in_off[b], n_in = in_off[b + 1] - x0, y0 = out_off[b];
    long n_out = resampled_length(n_in, L, M);
    n_out = n_out < out_off[b + 1] - y0 ? n_out : out_off[b + 1] - y0;     // never past the row's room
    const long n0 = (long)blockIdx.x * TN;
    if (n0 >= n_out) return;                                          // (the whole workgroup, before any barrier)
    const float* __restrict__ row = x + x0;
    auto src = [&](long j) -> float { return j >= 0 && j < n_in ? row[j] : 0.f; };
    resample_tile(n0, (int)(n_out - n0 < TN ? n_out - n0 : TN), L, M, K, TN, taps, src, y + y0 + n0, s_x, s_t);
}

// carry, consumed and produced are read and written here: no __restrict__ on them.
__global__ __launch_bounds__(RS_THREADS) void resample_stream_kernel(const float* __restrict__ chunk, long chunk_stride, RsLens lens, int flush_mask,
                                                                     const float* __restrict__ taps, int L, int M, int K, int TN, float* carry,
                                                                     int64_t* consumed, int64_t* produced, float* __restrict__ out, long out_stride) {
    __shared__ float s_x[RS_SPAN_FLOATS];
    __shared__ float s_t[RS_TAP_FLOATS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = b == 0 ? lens.n[0] : (b == 1 ? lens.n[1] : (b == 2 ? lens.n[2] : lens.n[3]));
    const bool flush = (flush_mask >> b) & 1;
    if (n == 0 && !flush) return;                                     // (the whole workgroup, before any barrier: the row keeps every bit)
    const long c0 = consumed[b], o0 = produced[b], c1 = c0 + n;
    long n_new = (flush ? resampled_length(c1, L, M) : resampled_ready(c1, L, M, K)) - o0;
    n_new = n_new < 0 ? 0 : (n_new > out_stride ? out_stride : n_new);     // (the host sized the row from the same integers)
    const float* __restrict__ ch = chunk + (long)b * chunk_stride;
    float* cr = carry + (long)b * (K - 1);
    // sample j of the row's signal from [carry | chunk]: the carry holds [c0 - (K - 1), c0) -- zeros in front of the signal, as the row was opened
    // --, the chunk [c0, c1); nothing older is ever read (an output that is not final yet starts after c0 - K), behind c1 the signal has ended
    auto src = [&](long j) -> float {
        if (j >= c1 || j < c0 - (K - 1)) return 0.f;
        return j >= c0 ? ch[j - c0] : cr[j - c0 + (K - 1)];
    };
    for (long t0 = 0; t0 < n_new; t0 += TN)
        resample_tile(o0 + t0, (int)(n_new - t0 < TN ? n_new - t0 : TN), L, M, K, TN, taps, src, out + (long)b * out_stride + t0, s_x, s_t);
    float keep[2];                                                    // K - 1 <= 511 <= 2 RS_THREADS: the new carry, read before anyone writes it
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + q * RS_THREADS;
        keep[q] = i < K - 1 ? src(c1 - (K - 1) + i) : 0.f;            // a chunk shorter than K - 1 keeps the old carry's tail
    }
    __syncthreads();                                                  // every thread has the counters and its part of the old carry
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int i = tid + q * RS_THREADS;
        if (i < K - 1) cr[i] = keep[q];
    }
    if (tid == 0) {
        consumed[b] = c1;
        produced[b] = o0 + n_new;
    }
}

}  // namespace tg

using namespace tg;

extern "C" int tg_resample(const float* x, const int64_t* in_off, const int64_t* out_off, int32_t B, int64_t max_out, const float* taps, int32_t L,
                           int32_t M, int32_t K, float* y, void* stream) {
    TG_REQUIRE(B >= 1 && B <= 65535 && max_out >= 1 && max_out <= ((int64_t)1 << 40) && geometry_ok(L, M, K),
               "tg_resample: outside the envelope 1 <= B <= 65535, max_out >= 1, 1 <= L <= %d, M >= 1, K even in [2, %d], a tile's span within %d "
               "samples (B=%d max_out=%lld L=%d M=%d K=%d)", RS_MAX_L, RS_MAX_K, RS_SPAN_FLOATS, B, (long long)max_out, L, M, K);
    TG_REQUIRE(x && in_off && out_off && taps && y, "tg_resample: null pointer");
    const int tn = tile_outputs(L, M, K);
    const int64_t tiles = (max_out + tn - 1) / tn;
    TG_REQUIRE(tiles <= 0x7fffffff, "tg_resample: outside the envelope: %lld tiles", (long long)tiles);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, B), dim3(RS_THREADS), 0, (hipStream_t)stream, x, in_off, out_off, taps, L, M, K, tn, y);
    return check_launch("tg_resample");
}

extern "C" int tg_resample_stream(const float* chunk, int64_t chunk_stride, int32_t n0, int32_t n1, int32_t n2, int32_t n3, int32_t flush_mask,
                                  const float* taps, int32_t L, int32_t M, int32_t K, float* carry, int64_t* consumed, int64_t* produced, float* out,
                                  int64_t out_stride, int32_t B, void* stream) {
    RsLens lens = {{n0, n1, n2, n3}};
    int64_t n_max = 0;
    bool rows_ok = B >= 1 && B <= RS_MAX_ROWS;
    for (int b = 0; b < RS_MAX_ROWS; ++b) {
        rows_ok = rows_ok && lens.n[b] >= 0 && (b < B || lens.n[b] == 0);
        n_max = lens.n[b] > n_max ? lens.n[b] : n_max;
    }
    TG_REQUIRE(rows_ok && flush_mask >= 0 && flush_mask < (1 << (rows_ok ? B : 1)) && (n_max >= 1 || flush_mask != 0) && geometry_ok(L, M, K) &&
                   chunk_stride >= n_max,
               "tg_resample_stream: outside the envelope 1 <= B <= %d, n[b] >= 0 (0 for b >= B), a row with samples or a flush bit below 2^B, 1 <= L "
               "<= %d, M >= 1, K even in [2, %d], chunk_stride >= max n (B=%d n=%d,%d,%d,%d flush_mask=%d L=%d M=%d K=%d chunk_stride=%lld)",
               RS_MAX_ROWS, RS_MAX_L, RS_MAX_K, B, n0, n1, n2, n3, flush_mask, L, M, K, (long long)chunk_stride);
    // the most a row can produce: ceil(n L / M) outputs become final in a push, a flush adds those whose span reaches up to K/2 samples past the end
    const int64_t need = ((n_max + (flush_mask ? K / 2 : 0)) * L + M - 1) / M + 1;
    TG_REQUIRE(out_stride >= need, "tg_resample_stream: outside the envelope out_stride >= ceil((max n + K/2 on a flush) L / M) + 1 = %lld "
               "(out_stride=%lld)", (long long)need, (long long)out_stride);
    TG_REQUIRE((chunk || n_max == 0) && taps && carry && consumed && produced && out, "tg_resample_stream: null pointer");
    hipLaunchKernelGGL(resample_stream_kernel, dim3(B), dim3(RS_THREADS), 0, (hipStream_t)stream, chunk, (long)chunk_stride, lens, flush_mask, taps, L, M, K,
                       tile_outputs(L, M, K), carry, consumed, produced, out, (long)out_stride);
    return check_launch("tg_resample_stream");
}
