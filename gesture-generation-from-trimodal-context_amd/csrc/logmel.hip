// Log-mel spectrogram of raw 16 kHz audio (utils/data_utils.py:34-38: librosa melspectrogram(n_fft 1024, hop 512, power 2), 128 Slaney mels,
// power_to_db(ref = max), fp16) in two launches.
//
// logmel_frame_kernel -- one 128-thread workgroup per (clip, frame):
//   1. thread t reads the 8 samples 2 (t + 128 r), 2 (t + 128 r) + 1 (r < 4) of its frame straight from the clip -- center = True is index
//      arithmetic (reflection or zeros), no padded copy exists -- and multiplies by the window: the 1024 real samples ARE the 512 complex
//      points z[n] = x[2n] + i x[2n + 1] of a half-length transform;
//   2. 512-point complex FFT, Stockham autosort (natural order out, no bit reversal): radix 4 at Ns = 1 (from registers), 4, 16, 64, then one
//      radix-2 stage; one butterfly per thread and stage, ping-pong between two LDS arrays, twiddles exp(-2 pi i k / 1024) read from an LDS copy
//      of the caller's table (fp64 values rounded once; no sincos anywhere);
//   3. real-input post-pass X[k] = E[k] + W^k O[k] and the 513 powers |X[k]|^2 into LDS;
//   4. thread i gathers mel filter i: 24 (zero-padded) weights times consecutive bins from the filter's first bin on, one fma chain in bin
//      order -- no atomics, a fixed summation order;
//   5. the workgroup's largest mel power goes to the workspace beside its 128 mel powers (stored frame-major: coalesced).
// logmel_db_kernel -- one workgroup per (32 frames, clip): the clip's maximum from the per-frame maxima (max of floats is exact in any order;
//   the order is fixed anyway), the dB formula, the -80 dB floor, the optional fp16 cast, and the transpose to (128, F) through an LDS tile.
//
// LDS: 2 x 544 float2 (FFT ping-pong; index i lives at i + i / 16, which spreads the stride-4 stores of the first stage over all banks)
// + 512 float2 twiddles + 2 floats = 12.8 KB per workgroup; the powers reuse the second FFT array.
#include "common.hpp"

namespace tg {

constexpr int LM_HOP = 512, LM_MELS = 128, LM_TAPS = 24, LM_THREADS = 128;
constexpr int LM_TAB_WIN = 1024, LM_TAB_W = 2048, LM_TAB_START = LM_TAB_W + LM_TAPS * LM_MELS, LM_TAB_FLOATS = LM_TAB_START + LM_MELS;
constexpr int LM_BUF = 512 + 512 / 16;
constexpr int LM_TILE_F = 32;

__device__ __forceinline__ int lm_pad(int i) { return i + (i >> 4); }
__device__ __forceinline__ float2 lm_cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 lm_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 lm_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// forward radix-4 butterfly of (v0 .. v3), results written Ns apart from j0
template <int NS>
__device__ __forceinline__ void lm_bfly4_store(float2 v0, float2 v1, float2 v2, float2 v3, float2* __restrict__ out, int j0) {
    const float2 a = lm_add(v0, v2), b = lm_sub(v0, v2), c = lm_add(v1, v3), d = lm_sub(v1, v3);
    const float2 dm = make_float2(d.y, -d.x);                 // -i d
    out[lm_pad(j0)] = lm_add(a, c);
    out[lm_pad(j0 + NS)] = lm_add(b, dm);
    out[lm_pad(j0 + 2 * NS)] = lm_sub(a, c);
    out[lm_pad(j0 + 3 * NS)] = lm_sub(b, dm);
}

// one radix-4 Stockham stage over 512 points with sub-transform length NS coming in: butterfly t of 128
template <int NS>
__device__ __forceinline__ void lm_stage4(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw, int t) {
    const int k = t & (NS - 1);
    const int m = k * (1024 / (NS * 4));                      // exp(-2 pi i r k / (4 NS)) = W1024^(r m), r m < 768
    float2 v0 = in[lm_pad(t)], v1 = in[lm_pad(t + 128)], v2 = in[lm_pad(t + 256)], v3 = in[lm_pad(t + 384)];
    v1 = lm_cmul(v1, tw[m]);
    v2 = lm_cmul(v2, tw[2 * m]);
    const int m3 = 3 * m;
    float2 w3 = tw[m3 & 511];
    if (m3 >= 512) w3 = make_float2(-w3.x, -w3.y);            // W1024^(k + 512) = -W1024^k
    v3 = lm_cmul(v3, w3);
    lm_bfly4_store<NS>(v0, v1, v2, v3, out, ((t - k) << 2) + k);
}

__global__ __launch_bounds__(LM_THREADS) void logmel_frame_kernel(const float* __restrict__ audio, long audio_stride, int L, int F, int reflect,
                                                                  const float* __restrict__ tab, float* __restrict__ mel,
                                                                  float* __restrict__ frame_max) {
    __shared__ float2 bufa[LM_BUF], bufb[LM_BUF], tw[512];
    __shared__ unsigned wmax[2];
    const int t = threadIdx.x, f = blockIdx.x, n = blockIdx.y;
    const float* __restrict__ clip = audio + (long)n * audio_stride;
    const float2* __restrict__ tab2 = reinterpret_cast<const float2*>(tab);
#pragma unroll
    for (int q = 0; q < 4; ++q) tw[t + 128 * q] = tab2[t + 128 * q];
    // stage 0 (Ns = 1, no twiddles) from registers
    float2 v[4];
    const long p0 = (long)f * LM_HOP - LM_HOP;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 2 * (t + 128 * r);
        const float2 w = tab2[(LM_TAB_WIN + i) >> 1];
        float x[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            long p = p0 + i + h;
            bool live = true;
            if (p < 0) { live = reflect != 0; p = -p; }
            else if (p >= L) { live = reflect != 0; p = 2 * (long)(L - 1) - p; }
            live = live && p >= 0 && p < L;                   // (the launcher admits reflection only for L >= 513, where this always holds)
            x[h] = live ? clip[p] : 0.f;
        }
        v[r] = make_float2(x[0] * w.x, x[1] * w.y);
    }
    lm_bfly4_store<1>(v[0], v[1], v[2], v[3], bufa, 4 * t);
    __syncthreads();
    lm_stage4<4>(bufa, bufb, tw, t);
    __syncthreads();
    lm_stage4<16>(bufb, bufa, tw, t);
    __syncthreads();
    lm_stage4<64>(bufa, bufb, tw, t);
    __syncthreads();
    // radix-2 stage, Ns = 256: butterflies t and t + 128
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int j = t + 128 * q;
        const float2 a = bufb[lm_pad(j)], b = lm_cmul(bufb[lm_pad(j + 256)], tw[2 * j]);
        bufa[lm_pad(j)] = lm_add(a, b);
        bufa[lm_pad(j + 256)] = lm_sub(a, b);
    }
    __syncthreads();
    // real-input post-pass: Z = FFT512(z) in bufa -> power of X[k], k <= 512
    float* __restrict__ pw = reinterpret_cast<float*>(bufb);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = t + 128 * q;
        const float2 zk = bufa[lm_pad(k)], zr = bufa[lm_pad((512 - k) & 511)];
        const float2 e = make_float2(0.5f * (zk.x + zr.x), 0.5f * (zk.y - zr.y));          // (Z[k] + conj Z[512 - k]) / 2
        const float2 d = make_float2(0.5f * (zk.x - zr.x), 0.5f * (zk.y + zr.y));          // (Z[k] - conj Z[512 - k]) / 2
        const float2 wd = lm_cmul(tw[k], d);
        const float re = e.x + wd.y, im = e.y - wd.x;                                       // E + W^k (d / i)
        pw[k] = re * re + im * im;
    }
    if (t == 0) {
        const float2 z0 = bufa[0];
        const float x = z0.x - z0.y;
        pw[512] = x * x;
    }
    __syncthreads();
    // mel filter t: bins s .. s + 23 (clamped; weights past the filter are zero)
    int s = (int)tab[LM_TAB_START + t];
    s = s < 0 ? 0 : (s > 512 ? 512 : s);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < LM_TAPS; ++j) {
        const int b = s + j > 512 ? 512 : s + j;
        acc = fmaf(tab[LM_TAB_W + j * LM_MELS + t], pw[b], acc);
    }
    mel[((long)n * F + f) * LM_MELS + t] = acc;
    const unsigned mx = wave_max_u32(__float_as_uint(fmaxf(acc, 0.f)));
    if ((t & 63) == 0) wmax[t >> 6] = mx;
    __syncthreads();
    if (t == 0) frame_max[(long)n * F + f] = __uint_as_float(wmax[0] > wmax[1] ? wmax[0] : wmax[1]);
}

template <typename TO>
__global__ __launch_bounds__(256) void logmel_db_kernel(const float* __restrict__ mel, const float* __restrict__ frame_max, int F, TO* __restrict__ out) {
    __shared__ float red[256];
    __shared__ float tile[LM_TILE_F][LM_MELS + 1];
    const int t = threadIdx.x, n = blockIdx.y, f0 = blockIdx.x * LM_TILE_F;
    float m = 0.f;
    for (int q = t; q < F; q += 256) m = fmaxf(m, frame_max[(long)n * F + q]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    const float ref_log = log10f(fmaxf(red[0], 1e-10f));
#pragma unroll
    for (int q = 0; q < LM_TILE_F * LM_MELS / 256; ++q) {
        const int e = t + 256 * q, fr = e >> 7, ml = e & 127;
        if (f0 + fr < F) tile[fr][ml] = mel[((long)n * F + f0 + fr) * LM_MELS + ml];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LM_TILE_F * LM_MELS / 256; ++q) {
        const int e = t + 256 * q, ml = e >> 5, fr = e & 31;
        if (f0 + fr < F) {
            // 10 (log10 M - log10 max M): the difference is formed first (a product-then-subtract would be contracted into an fma and leave the
            // product's rounding error on the clip's largest entry), so that entry gives exactly 0 and max(db) - 80 is -80; min(., 0) keeps
            // that true whatever log10f's last bit does
            const float db = fminf(10.f * (log10f(fmaxf(tile[fr][ml], 1e-10f)) - ref_log), 0.f);
            out[((long)n * LM_MELS + ml) * F + f0 + fr] = (TO)fmaxf(db, -80.f);
        }
    }
}

static int lm_check(const char* who, int32_t N, int32_t L, int64_t& F) {
    TG_REQUIRE(N >= 1 && N <= 65535, "%s: N = %d clips, 1 .. 65535 supported", who, (int)N);
    TG_REQUIRE(L >= 1 && L <= (1 << 30), "%s: L = %d samples, 1 .. 2^30 supported", who, (int)L);
    F = 1 + L / LM_HOP;
    return 0;
}

}  // namespace tg

using namespace tg;

extern "C" int tg_logmel_query(int32_t N, int32_t L, int64_t* sizes) {
    TG_REQUIRE(sizes, "tg_logmel_query: sizes is NULL");
    int64_t F;
    if (int e = lm_check("tg_logmel_query", N, L, F)) return e;
    sizes[0] = F;
    sizes[1] = LM_TAB_FLOATS;
    sizes[2] = (int64_t)N * F * (LM_MELS + 1) * (int64_t)sizeof(float);
    return 0;
}

extern "C" int tg_logmel(const float* audio, int64_t audio_stride, int32_t N, int32_t L, int32_t pad_mode, const float* tables, int64_t table_floats,
                         void* ws, int64_t ws_bytes, void* out, int32_t out_half, void* stream) {
    TG_REQUIRE(audio && tables && ws && out, "tg_logmel: NULL pointer argument");
    int64_t F;
    if (int e = lm_check("tg_logmel", N, L, F)) return e;
    TG_REQUIRE(pad_mode == 0 || pad_mode == 1, "tg_logmel: pad_mode %d unknown (0 = reflect, 1 = constant)", (int)pad_mode);
    TG_REQUIRE(pad_mode != 0 || L >= LM_HOP + 1, "tg_logmel: reflect padding needs at least %d samples, got %d (use pad_mode 1 = constant)", LM_HOP + 1, (int)L);
    TG_REQUIRE(out_half == 0 || out_half == 1, "tg_logmel: out_half must be 0 or 1");
    TG_REQUIRE(audio_stride >= L || N == 1, "tg_logmel: audio_stride %lld < L = %d", (long long)audio_stride, (int)L);
    TG_REQUIRE(table_floats >= LM_TAB_FLOATS, "tg_logmel: table of %lld floats, %d needed (tg_logmel_query)", (long long)table_floats, LM_TAB_FLOATS);
    const int64_t need = (int64_t)N * F * (LM_MELS + 1) * (int64_t)sizeof(float);
    TG_REQUIRE(ws_bytes >= need, "tg_logmel: workspace of %lld bytes, %lld needed (tg_logmel_query)", (long long)ws_bytes, (long long)need);
    TG_REQUIRE(aligned16(tables) && aligned16(ws) && (reinterpret_cast<uintptr_t>(audio) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(out) & (out_half ? 1u : 3u)) == 0, "tg_logmel: misaligned pointer (tables / ws 16 bytes)");
    hipStream_t s = (hipStream_t)stream;
    float* mel = static_cast<float*>(ws);
    float* frame_max = mel + (int64_t)N * F * LM_MELS;
    hipLaunchKernelGGL(logmel_frame_kernel, dim3((unsigned)F, (unsigned)N), dim3(LM_THREADS), 0, s, audio, (long)audio_stride, (int)L, (int)F,
                       pad_mode == 0 ? 1 : 0, tables, mel, frame_max);
    if (check_launch("tg_logmel(frames)")) return 1;
    const dim3 grid((unsigned)cdiv(F, LM_TILE_F), (unsigned)N);
    if (out_half)
        hipLaunchKernelGGL(logmel_db_kernel<_Float16>, grid, dim3(256), 0, s, (const float*)mel, (const float*)frame_max, (int)F, static_cast<_Float16*>(out));
    else
        hipLaunchKernelGGL(logmel_db_kernel<float>, grid, dim3(256), 0, s, (const float*)mel, (const float*)frame_max, (int)F, static_cast<float*>(out));
    return check_launch("tg_logmel(db)");
}
