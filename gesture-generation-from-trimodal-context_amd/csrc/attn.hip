// Bahdanau attention of the Seq2Seq decoder (model/seq2seq_net.py:59-89, 165-167), one decoder step per launch.
//
//   e[b,t,:] = tanh(q[b] + keys[b,t,:])      q = h_top W_h^T (per step), keys = enc W_e^T + b_a (once per forward), both by tg_gemm_nt
//   s[b,t]   = v . e[b,t,:]
//   w[b,:]   = softmax over ALL Te positions (the reference does not mask padded positions, where enc is zero; neither does this)
//   ctx[b,:] = sum_t w[b,t] enc[b,t,:]
//
// One 256-thread workgroup owns one batch row in both directions: no workgroup waits on another, the backward's "+=" into the row's
// accumulators needs no atomics, and every sum runs in a fixed order (results are bit-identical from run to run).  A row's working set is
// 2 Te H floats (54 KB at Te = 34, H = 200): it is read once per launch with 16-byte loads and stays in L2 between the steps.
// Two thread maps are used: "wave per position" (a wave walks the H channels of one t with float4 lanes and reduces across lanes) for the
// sums over channels, and "(group, channel quad)" (thread (g, j4) walks t = g, g + G, ... for one float4 of channels, the G partials are
// combined through LDS in group order) for the sums over positions.
#include "common.hpp"

namespace tg {

constexpr int ATTN_THREADS = 256, ATTN_WAVES = ATTN_THREADS / 64, ATTN_MAX_TE = 128, ATTN_MAX_H = 320;
#define ATTN_ENVELOPE "B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320"

inline bool attn_in_envelope(int64_t B, int64_t Te, int64_t H) {
    return B >= 1 && Te >= 1 && Te <= ATTN_MAX_TE && H >= 8 && H <= ATTN_MAX_H && H % 4 == 0;
}

__device__ __forceinline__ float attn_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ float attn_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 x) { *reinterpret_cast<f32x4*>(p) = x; }

__global__ __launch_bounds__(ATTN_THREADS) void attn_step_fwd_kernel(const float* __restrict__ q, const float* __restrict__ keys,
                                                                     const float* __restrict__ enc, const float* __restrict__ v,
                                                                     float* __restrict__ w, float* __restrict__ ctx, long ctx_ld, int Te, int H) {
    __shared__ __attribute__((aligned(16))) float s_q[ATTN_MAX_H], s_v[ATTN_MAX_H], s_w[ATTN_MAX_TE], s_part[ATTN_THREADS * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x, nj4 = H >> 2;
    const float* kb = keys + (long)b * Te * H;
    const float* eb = enc + (long)b * Te * H;
    for (int j = tid; j < H; j += ATTN_THREADS) { s_q[j] = q[(long)b * H + j]; s_v[j] = v[j]; }
    __syncthreads();
    // scores: wave per position
    for (int t = wv; t < Te; t += ATTN_WAVES) {
        float a = 0.f;
        for (int j4 = lane; j4 < nj4; j4 += 64) {
            const f32x4 k = ld4(kb + (long)t * H + 4 * j4), qq = ld4(s_q + 4 * j4), vv = ld4(s_v + 4 * j4);
#pragma unroll
            for (int c = 0; c < 4; ++c) a += vv[c] * tanhf(qq[c] + k[c]);
        }
        a = attn_wave_sum(a);
        if (lane == 0) s_w[t] = a;
    }
    __syncthreads();
    // softmax over all Te positions: wave 0, lane l holds t = l and l + 64
    if (wv == 0) {
        const float s0 = lane < Te ? s_w[lane] : -INFINITY, s1 = lane + 64 < Te ? s_w[lane + 64] : -INFINITY;
        const float mx = attn_wave_max(fmaxf(s0, s1));
        const float e0 = lane < Te ? expf(s0 - mx) : 0.f, e1 = lane + 64 < Te ? expf(s1 - mx) : 0.f;
        const float sum = attn_wave_sum(e0 + e1);
        if (lane < Te) { const float x = e0 / sum; s_w[lane] = x; w[(long)b * Te + lane] = x; }
        if (lane + 64 < Te) { const float x = e1 / sum; s_w[lane + 64] = x; w[(long)b * Te + lane + 64] = x; }
    }
    __syncthreads();
    // context: (group, channel quad)
    const int G = ATTN_THREADS / nj4 < Te ? ATTN_THREADS / nj4 : Te;      // >= 1 (nj4 <= 80), <= 128
    const int g = tid / nj4, j4 = tid - g * nj4;
    if (g < G) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int t = g; t < Te; t += G) {
            const f32x4 x = ld4(eb + (long)t * H + 4 * j4);
            const float wt = s_w[t];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(wt, x[c], acc[c]);
        }
        st4(s_part + ((long)g * nj4 + j4) * 4, acc);                        // [g][H]
    }
    __syncthreads();
    for (int j = tid; j < H; j += ATTN_THREADS) {
        float a = s_part[j];
        for (int gg = 1; gg < G; ++gg) a += s_part[gg * H + j];
        ctx[(long)b * ctx_ld + j] = a;
    }
}

__global__ __launch_bounds__(ATTN_THREADS) void attn_step_bwd_kernel(const float* __restrict__ dctx, long dctx_ld, const float* __restrict__ q,
                                                                     const float* __restrict__ w, const float* __restrict__ keys,
                                                                     const float* __restrict__ enc, const float* __restrict__ v,
                                                                     float* __restrict__ dq, float* __restrict__ dkeys_acc,
                                                                     float* __restrict__ denc_acc, float* __restrict__ dv_rows, int Te, int H) {
    __shared__ __attribute__((aligned(16))) float s_q[ATTN_MAX_H], s_v[ATTN_MAX_H], s_dc[ATTN_MAX_H], s_w[ATTN_MAX_TE], s_ds[ATTN_MAX_TE],
        s_pq[ATTN_THREADS * 4], s_pv[ATTN_THREADS * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x, nj4 = H >> 2;
    const long row = (long)b * Te * H;
    for (int j = tid; j < H; j += ATTN_THREADS) { s_q[j] = q[(long)b * H + j]; s_v[j] = v[j]; s_dc[j] = dctx[(long)b * dctx_ld + j]; }
    for (int t = tid; t < Te; t += ATTN_THREADS) s_w[t] = w[(long)b * Te + t];
    __syncthreads();
    // dw_t = dctx . enc_t and denc_t += w_t dctx: wave per position
    for (int t = wv; t < Te; t += ATTN_WAVES) {
        const float wt = s_w[t];
        float a = 0.f;
        for (int j4 = lane; j4 < nj4; j4 += 64) {
            const long o = row + (long)t * H + 4 * j4;
            const f32x4 x = ld4(enc + o), d = ld4(s_dc + 4 * j4);
            f32x4 acc = ld4(denc_acc + o);
#pragma unroll
            for (int c = 0; c < 4; ++c) { a = fmaf(d[c], x[c], a); acc[c] = fmaf(wt, d[c], acc[c]); }
            st4(denc_acc + o, acc);
        }
        a = attn_wave_sum(a);
        if (lane == 0) s_ds[t] = a;
    }
    __syncthreads();
    // ds_t = w_t (dw_t - sum_u w_u dw_u): wave 0
    if (wv == 0) {
        const float w0 = lane < Te ? s_w[lane] : 0.f, w1 = lane + 64 < Te ? s_w[lane + 64] : 0.f;
        const float d0 = lane < Te ? s_ds[lane] : 0.f, d1 = lane + 64 < Te ? s_ds[lane + 64] : 0.f;
        const float dot = attn_wave_sum(fmaf(w0, d0, w1 * d1));
        if (lane < Te) s_ds[lane] = w0 * (d0 - dot);
        if (lane + 64 < Te) s_ds[lane + 64] = w1 * (d1 - dot);
    }
    __syncthreads();
    // e recomputed; da = ds v (1 - e^2): dkeys += da, dq = sum_t da, dv += sum_t ds e: (group, channel quad)
    const int G = ATTN_THREADS / nj4 < Te ? ATTN_THREADS / nj4 : Te;
    const int g = tid / nj4, j4 = tid - g * nj4;
    if (g < G) {
        const f32x4 qq = ld4(s_q + 4 * j4), vv = ld4(s_v + 4 * j4);
        f32x4 aq = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
        for (int t = g; t < Te; t += G) {
            const long o = row + (long)t * H + 4 * j4;
            const f32x4 k = ld4(keys + o);
            f32x4 dk = ld4(dkeys_acc + o);
            const float ds = s_ds[t];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float e = tanhf(qq[c] + k[c]);
                const float da = ds * vv[c] * (1.f - e * e);
                dk[c] += da; aq[c] += da; av[c] = fmaf(ds, e, av[c]);
            }
            st4(dkeys_acc + o, dk);
        }
        st4(s_pq + ((long)g * nj4 + j4) * 4, aq);
        st4(s_pv + ((long)g * nj4 + j4) * 4, av);
    }
    __syncthreads();
    for (int j = tid; j < H; j += ATTN_THREADS) {
        float a = s_pq[j], c = s_pv[j];
        for (int gg = 1; gg < G; ++gg) { a += s_pq[gg * H + j]; c += s_pv[gg * H + j]; }
        dq[(long)b * H + j] = a;
        dv_rows[(long)b * H + j] += c;
    }
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_attn_step_supported(int32_t B, int32_t Te, int32_t H, int32_t* supported) {
    TG_REQUIRE(supported, "tg_attn_step_supported: null pointer");
    TG_REQUIRE(B > 0 && Te > 0 && H > 0, "tg_attn_step_supported: sizes must be positive (B=%d Te=%d H=%d)", B, Te, H);
    *supported = attn_in_envelope(B, Te, H) ? 1 : 0;
    return 0;
}

int tg_attn_step_forward(const float* q, const float* keys, const float* enc, const float* v, float* w, float* ctx, int64_t ctx_ld, int32_t B,
                         int32_t Te, int32_t H, void* stream) {
    TG_REQUIRE(attn_in_envelope(B, Te, H), "tg_attn_step_forward: outside the envelope " ATTN_ENVELOPE " (B=%d Te=%d H=%d)", B, Te, H);
    TG_REQUIRE(q && keys && enc && v && w && ctx, "tg_attn_step_forward: null pointer");
    TG_REQUIRE(ctx_ld >= H, "tg_attn_step_forward: ctx row stride %lld < H = %d", (long long)ctx_ld, H);
    TG_REQUIRE(aligned16(keys) && aligned16(enc), "tg_attn_step_forward: keys / enc must be 16-byte aligned");
    hipLaunchKernelGGL(attn_step_fwd_kernel, dim3(B), dim3(ATTN_THREADS), 0, (hipStream_t)stream, q, keys, enc, v, w, ctx, (long)ctx_ld, Te, H);
    return check_launch("tg_attn_step_forward");
}

int tg_attn_step_backward(const float* dctx, int64_t dctx_ld, const float* q, const float* w, const float* keys, const float* enc, const float* v,
                          float* dq, float* dkeys_acc, float* denc_acc, float* dv_rows, int32_t B, int32_t Te, int32_t H, void* stream) {
    TG_REQUIRE(attn_in_envelope(B, Te, H), "tg_attn_step_backward: outside the envelope " ATTN_ENVELOPE " (B=%d Te=%d H=%d)", B, Te, H);
    TG_REQUIRE(dctx && q && w && keys && enc && v && dq && dkeys_acc && denc_acc && dv_rows, "tg_attn_step_backward: null pointer");
    TG_REQUIRE(dctx_ld >= H, "tg_attn_step_backward: dctx row stride %lld < H = %d", (long long)dctx_ld, H);
    TG_REQUIRE(aligned16(keys) && aligned16(enc) && aligned16(dkeys_acc) && aligned16(denc_acc),
               "tg_attn_step_backward: keys / enc / dkeys_acc / denc_acc must be 16-byte aligned");
    hipLaunchKernelGGL(attn_step_bwd_kernel, dim3(B), dim3(ATTN_THREADS), 0, (hipStream_t)stream, dctx, (long)dctx_ld, q, w, keys, enc, v, dq,
                       dkeys_acc, denc_acc, dv_rows, Te, H);
    return check_launch("tg_attn_step_backward");
}

}  // extern "C"
