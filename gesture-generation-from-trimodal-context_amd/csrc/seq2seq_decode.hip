// The eval-mode decoder loop of the Seq2Seq baseline (model/seq2seq_net.py:241-252) in ONE launch, one workgroup per batch row.
//
// In eval mode nothing couples one batch row to another: BatchNorm on running statistics is a per-channel affine map, dropout is off and the
// attention is already row-local.  A workgroup therefore owns its row for all n_frames - 1 decoded frames: no workgroup waits on another, the
// whole state (hidden states, concatenated pre_linear input, attention weights, gate pre-activations) lives in LDS, and the weights are
// re-read from L2 every frame (2.3 MB per frame at H = 200, 2 layers).  Per frame:
//
//   q = W_h h_top;  s_t = v . tanh(q + keys_t);  w = softmax over the row's first te_len[b] positions (NULL: all Te);  ctx = sum_t w_t enc_t
//   x = [pose ; z ; ctx ; speaker];  a = relu(scale * (W_pre x + b_pre) + shift)        (scale / shift: BatchNorm folded once in the prologue)
//   the n_layers GRU cells (gru_cell_fwd of gru_step.hpp);  out = W_out h_top + b_out;  next pose = seed pose t while t < n_pre, else out
//
// The products are matrix-vector products: a quarter wave per output row, 4 DEC_RU rows of a wave in flight at once, float4 lanes over K between a
// scalar head and a scalar tail -- a weight row may start at any 4-byte boundary (W_pre rows are 227 floats long at the reference
// configuration, W_h is the left half of W_a).  Every sum runs in a fixed order that depends on the weights' addresses and the row's own
// te_len only: a row's result does not depend on B, on its position in the batch or on other rows, and two runs are bit-identical.
#include "common.hpp"
#include "gru_step.hpp"

namespace tg {

constexpr int DEC_THREADS = 512, DEC_WAVES = DEC_THREADS / 64, DEC_RU = 4, DEC_JU = 4;
constexpr int DEC_MAX_TE = 128, DEC_MAX_H = 320, DEC_MAX_LAYERS = 4, DEC_MAX_W = 1024;
#define DEC_ENVELOPE                                                                                                                         \
    "B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320, 1 <= n_layers <= 4, n_frames >= 2, 0 <= n_pre <= n_frames, Po == Pd or n_frames == 2, " \
    "Z >= 0, S8 >= 0, 1 <= Po <= Pd, Pd + Z + H + S8 <= 1024"

inline bool dec_in_envelope(int64_t B, int64_t Te, int64_t H, int64_t nl, int64_t n_frames, int64_t n_pre, int64_t Pd, int64_t Po, int64_t Z,
                            int64_t S8) {
    return B >= 1 && Te >= 1 && Te <= DEC_MAX_TE && H >= 8 && H <= DEC_MAX_H && H % 4 == 0 && nl >= 1 && nl <= DEC_MAX_LAYERS && n_frames >= 2 &&
           n_pre >= 0 && n_pre <= n_frames && Pd >= 1 && Po >= 1 && Po <= Pd && (Po == Pd || n_frames == 2) && Z >= 0 && S8 >= 0 &&
           Z <= DEC_MAX_W && S8 <= DEC_MAX_W && Pd <= DEC_MAX_W && Pd + Z + H + S8 <= DEC_MAX_W;
}

struct DecArgs {
    const float *enc, *keys;
    const long long* te_len;
    const float *h0, *poses;
    long pose_bs;
    const float *z, *spk, *w_attn, *v, *w_pre, *b_pre, *gamma, *beta, *rmean, *rvar;
    float eps;
    const float *w_ih[DEC_MAX_LAYERS], *w_hh[DEC_MAX_LAYERS], *b_ih[DEC_MAX_LAYERS], *b_hh[DEC_MAX_LAYERS];
    const float *w_out, *b_out;
    float *outputs, *h_n, *attn_w;
    int B, Te, H, nl, n_frames, n_pre, Pd, Po, Z, S8;
};

__device__ __forceinline__ float dec_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__device__ __forceinline__ float dec_wave_max(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    return x;
}
__device__ __forceinline__ f32x4 dec_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// store(r, W[r, :K] . x + bias[r]) for r < rows.  W rows are ldw floats apart and start at any 4-byte boundary; x lies in LDS.  A quarter
// wave (16 lanes) owns an output row, so a wave takes 4 DEC_RU consecutive rows at a time; a lane issues the 16-byte loads of DEC_JU pieces of
// each of its DEC_RU rows together, the row's 16 partial sums meet in a four-step exchange, lane 0 of the quarter stores.
template <typename F>
__device__ __forceinline__ void dec_matvec(const float* __restrict__ W, long ldw, int rows, int K, const float* x, const float* __restrict__ bias,
                                           int wave, int lane, F store) {
    const int sub = lane >> 4, l16 = lane & 15;
    for (int r0 = wave * (4 * DEC_RU); r0 < rows; r0 += DEC_WAVES * 4 * DEC_RU) {
        const float* wr[DEC_RU];
        int head[DEC_RU];
        float acc[DEC_RU], bv[DEC_RU];
#pragma unroll
        for (int u = 0; u < DEC_RU; ++u) {
            const int rr = r0 + 4 * u + sub;
            const int r = rr < rows ? rr : rows - 1;                 // a row past the end repeats the last one and is not stored
            wr[u] = W + (long)r * ldw;
            const int h = (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(wr[u]) >> 2) & 3u)) & 3u);
            head[u] = h < K ? h : K;
            bv[u] = bias ? bias[r] : 0.f;
            acc[u] = l16 < head[u] ? wr[u][l16] * x[l16] : 0.f;
        }
        for (int jb = 0; 4 * jb < K; jb += 16 * DEC_JU) {
            f32x4 w[DEC_RU][DEC_JU];
#pragma unroll
            for (int u = 0; u < DEC_RU; ++u)
#pragma unroll
                for (int v = 0; v < DEC_JU; ++v) {
                    const int k = head[u] + 4 * (jb + 16 * v + l16);
                    w[u][v] = k + 4 <= K ? dec_ld4(wr[u] + k) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
            for (int u = 0; u < DEC_RU; ++u)
#pragma unroll
                for (int v = 0; v < DEC_JU; ++v) {
                    const int k = head[u] + 4 * (jb + 16 * v + l16);
                    if (k + 4 <= K) {
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[u] = fmaf(w[u][v][c], x[k + c], acc[u]);
                    }
                }
        }
#pragma unroll
        for (int u = 0; u < DEC_RU; ++u) {
            const int k = head[u] + 4 * ((K - head[u]) >> 2) + l16;     // at most 3 elements are left
            if (k < K) acc[u] = fmaf(wr[u][k], x[k], acc[u]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, 64);
            const int rr = r0 + 4 * u + sub;
            if (l16 == 0 && rr < rows) store(rr, acc[u] + bv[u]);
        }
    }
}

__global__ __launch_bounds__(DEC_THREADS) void seq2seq_decode_kernel(const DecArgs a) {
    __shared__ __attribute__((aligned(16))) float s_h[DEC_MAX_LAYERS][DEC_MAX_H], s_x[DEC_MAX_W], s_out[DEC_MAX_W], s_q[DEC_MAX_H], s_v[DEC_MAX_H],
        s_scale[DEC_MAX_H], s_shift[DEC_MAX_H], s_act[DEC_MAX_H], s_gi[3 * DEC_MAX_H], s_gh[3 * DEC_MAX_H], s_w[DEC_MAX_TE], s_part[DEC_THREADS * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    const int B = a.B, Te = a.Te, H = a.H, nl = a.nl, Pd = a.Pd, Po = a.Po, nj4 = H >> 2;
    const int c0 = Pd + a.Z, Lin = c0 + H + a.S8, S = a.n_frames - 1;
    int len = Te;
    if (a.te_len) {                                                  // validated on the host; clamped here so that no index can leave the row
        const long long v = a.te_len[b];
        len = v < 1 ? 1 : (v > Te ? Te : (int)v);
    }
    const float* kb = a.keys + (long)b * Te * H;
    const float* eb = a.enc + (long)b * Te * H;
    const float* pb = a.poses + (long)b * a.pose_bs;
    float* ob = a.outputs + (long)b * a.n_frames * Po;

    // ---- prologue: state, constants, BatchNorm folded to scale / shift, frame 0
    float bh[DEC_MAX_LAYERS][3];
#pragma unroll
    for (int l = 0; l < DEC_MAX_LAYERS; ++l) {
#pragma unroll
        for (int g = 0; g < 3; ++g) bh[l][g] = (l < nl && tid < H) ? a.b_hh[l][g * H + tid] : 0.f;
        if (l < nl && tid < H) s_h[l][tid] = a.h0[((long)l * B + b) * H + tid];
    }
    if (tid < H) {
        s_v[tid] = a.v[tid];
        const float sc = a.gamma[tid] / sqrtf(a.rvar[tid] + a.eps);
        s_scale[tid] = sc;
        s_shift[tid] = a.beta[tid] - a.rmean[tid] * sc;
    }
    for (int j = tid; j < Pd; j += DEC_THREADS) s_x[j] = pb[j];
    for (int j = tid; j < a.Z; j += DEC_THREADS) s_x[Pd + j] = a.z[(long)b * a.Z + j];
    for (int j = tid; j < a.S8; j += DEC_THREADS) s_x[c0 + H + j] = a.spk[(long)b * a.S8 + j];
    for (int j = tid; j < Po; j += DEC_THREADS) ob[j] = pb[j];       // Po <= Pd (Po == Pd, or one decoded frame)
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int t = s + 1;
        // ---- q = W_h h_top  (W_h: the left H columns of W_a [H][2H])
        dec_matvec(a.w_attn, 2L * H, H, H, s_h[nl - 1], nullptr, wv, lane, [&](int r, float y) { s_q[r] = y; });
        __syncthreads();
        // ---- scores: wave per position
        for (int p = wv; p < len; p += DEC_WAVES) {
            float sc = 0.f;
            for (int j4 = lane; j4 < nj4; j4 += 64) {
                const f32x4 k = dec_ld4(kb + (long)p * H + 4 * j4), qq = dec_ld4(s_q + 4 * j4), vv = dec_ld4(s_v + 4 * j4);
#pragma unroll
                for (int c = 0; c < 4; ++c) sc += vv[c] * tanhf(qq[c] + k[c]);
            }
            sc = dec_wave_sum(sc);
            if (lane == 0) s_w[p] = sc;
        }
        __syncthreads();
        // ---- softmax over the row's len positions: wave 0, lane l holds p = l and l + 64; exact zeros past len
        if (wv == 0) {
            const float s0 = lane < len ? s_w[lane] : -INFINITY, s1 = lane + 64 < len ? s_w[lane + 64] : -INFINITY;
            const float mx = dec_wave_max(fmaxf(s0, s1));
            const float e0 = lane < len ? expf(s0 - mx) : 0.f, e1 = lane + 64 < len ? expf(s1 - mx) : 0.f;
            const float sum = dec_wave_sum(e0 + e1);
            const float x0 = e0 / sum, x1 = e1 / sum;
            s_w[lane] = x0; s_w[lane + 64] = x1;
            if (a.attn_w) {
                float* wo = a.attn_w + ((long)s * B + b) * Te;
                if (lane < Te) wo[lane] = x0;
                if (lane + 64 < Te) wo[lane + 64] = x1;
            }
        }
        __syncthreads();
        // ---- context: (group, channel quad), partials added in group order
        const int G = DEC_THREADS / nj4 < len ? DEC_THREADS / nj4 : len;        // >= 1, G * H <= 4 DEC_THREADS
        {
            const int g = tid / nj4, j4 = tid - g * nj4;
            if (g < G) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int p = g; p < len; p += G) {
                    const f32x4 x = dec_ld4(eb + (long)p * H + 4 * j4);
                    const float wt = s_w[p];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = fmaf(wt, x[c], acc[c]);
                }
                *reinterpret_cast<f32x4*>(s_part + ((long)g * nj4 + j4) * 4) = acc;
            }
        }
        __syncthreads();
        if (tid < H) {
            float c = s_part[tid];
            for (int gg = 1; gg < G; ++gg) c += s_part[gg * H + tid];
            s_x[c0 + tid] = c;
        }
        __syncthreads();
        // ---- pre_linear: Linear, BatchNorm on running statistics, ReLU
        dec_matvec(a.w_pre, (long)Lin, H, Lin, s_x, a.b_pre, wv, lane, [&](int r, float y) { s_act[r] = fmaxf(fmaf(s_scale[r], y, s_shift[r]), 0.f); });
        __syncthreads();
        // ---- the GRU stack, one step from the previous state
#pragma unroll
        for (int l = 0; l < DEC_MAX_LAYERS; ++l) {
            if (l < nl) {
                const float* xin = l == 0 ? s_act : s_h[l > 0 ? l - 1 : 0];
                dec_matvec(a.w_ih[l], (long)H, 3 * H, H, xin, a.b_ih[l], wv, lane, [&](int r, float y) { s_gi[r] = y; });
                dec_matvec(a.w_hh[l], (long)H, 3 * H, H, s_h[l], nullptr, wv, lane, [&](int r, float y) { s_gh[r] = y; });
                __syncthreads();
                if (tid < H) {
                    const float gh[3] = {s_gh[tid], s_gh[H + tid], s_gh[2 * H + tid]};
                    const GruCell c = gru_cell_fwd(s_gi[tid], s_gi[H + tid], s_gi[2 * H + tid], gh, bh[l][0], bh[l][1], bh[l][2], s_h[l][tid]);
                    s_h[l][tid] = c.h;
                }
                __syncthreads();
            }
        }
        // ---- out = W_out h_top + b_out; the next input pose
        dec_matvec(a.w_out, (long)H, Po, H, s_h[nl - 1], a.b_out, wv, lane, [&](int r, float y) { s_out[r] = y; });
        __syncthreads();
        for (int j = tid; j < Po; j += DEC_THREADS) ob[(long)t * Po + j] = s_out[j];
        if (t < S) {                                                  // (Po == Pd here: more than one decoded frame)
            for (int j = tid; j < Pd; j += DEC_THREADS) s_x[j] = t < a.n_pre ? pb[(long)t * Pd + j] : s_out[j];
        }
        // (s_x, s_out and s_h are next read or written behind the barriers of the next frame)
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < DEC_MAX_LAYERS; ++l)
        if (l < nl && tid < H) a.h_n[((long)l * B + b) * H + tid] = s_h[l][tid];
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_seq2seq_decode_supported(int32_t B, int32_t Te, int32_t H, int32_t n_layers, int32_t n_frames, int32_t n_pre, int32_t Pd, int32_t Po,
                                int32_t Z, int32_t S8, int32_t* supported) {
    TG_REQUIRE(supported, "tg_seq2seq_decode_supported: null pointer");
    TG_REQUIRE(B > 0 && Te > 0 && H > 0 && n_layers > 0 && n_frames > 0 && Pd > 0 && Po > 0 && n_pre >= 0 && Z >= 0 && S8 >= 0,
               "tg_seq2seq_decode_supported: sizes must be positive (B=%d Te=%d H=%d n_layers=%d n_frames=%d n_pre=%d Pd=%d Po=%d Z=%d S8=%d)", B, Te,
               H, n_layers, n_frames, n_pre, Pd, Po, Z, S8);
    *supported = dec_in_envelope(B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z, S8) ? 1 : 0;
    return 0;
}

int tg_seq2seq_decode_eval(const float* enc, const float* keys, const void* te_len, const float* h0, const float* poses, int32_t pose_frames,
                           const float* z, const float* spk, const float* w_attn, const float* v, const float* w_pre, const float* b_pre,
                           const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                           const void* const* gru_params, const float* w_out, const float* b_out, float* outputs, float* h_n, float* attn_w,
                           int32_t B, int32_t Te, int32_t H, int32_t n_layers, int32_t n_frames, int32_t n_pre, int32_t Pd, int32_t Po, int32_t Z,
                           int32_t S8, void* stream) {
    TG_REQUIRE(dec_in_envelope(B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z, S8),
               "tg_seq2seq_decode_eval: outside the envelope " DEC_ENVELOPE " (B=%d Te=%d H=%d n_layers=%d n_frames=%d n_pre=%d Pd=%d Po=%d Z=%d S8=%d)",
               B, Te, H, n_layers, n_frames, n_pre, Pd, Po, Z, S8);
    TG_REQUIRE(pose_frames >= 1 && pose_frames >= n_pre, "tg_seq2seq_decode_eval: poses holds %d frames, max(n_pre, 1) = %d are read", pose_frames,
               n_pre > 1 ? n_pre : 1);
    TG_REQUIRE(enc && keys && h0 && poses && w_attn && v && w_pre && b_pre && bn_gamma && bn_beta && bn_mean && bn_var && gru_params && w_out &&
                   b_out && outputs && h_n,
               "tg_seq2seq_decode_eval: null pointer");
    TG_REQUIRE((Z == 0 || z) && (S8 == 0 || spk), "tg_seq2seq_decode_eval: Z = %d / S8 = %d without their tensors", Z, S8);
    TG_REQUIRE(aligned16(keys) && aligned16(enc), "tg_seq2seq_decode_eval: keys / enc must be 16-byte aligned");
    DecArgs a;
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < n_layers; ++l) {          // the table holds 4 n_layers entries: w_ih, w_hh, b_ih, b_hh of layer 0, then layer 1, ...
        a.w_ih[l] = (const float*)gru_params[4 * l]; a.w_hh[l] = (const float*)gru_params[4 * l + 1];
        a.b_ih[l] = (const float*)gru_params[4 * l + 2]; a.b_hh[l] = (const float*)gru_params[4 * l + 3];
        TG_REQUIRE(a.w_ih[l] && a.w_hh[l] && a.b_ih[l] && a.b_hh[l], "tg_seq2seq_decode_eval: null GRU parameter of layer %d", l);
    }
    a.enc = enc; a.keys = keys; a.te_len = (const long long*)te_len; a.h0 = h0; a.poses = poses; a.pose_bs = (long)pose_frames * Pd;
    a.z = z; a.spk = spk; a.w_attn = w_attn; a.v = v; a.w_pre = w_pre; a.b_pre = b_pre;
    a.gamma = bn_gamma; a.beta = bn_beta; a.rmean = bn_mean; a.rvar = bn_var; a.eps = bn_eps;
    a.w_out = w_out; a.b_out = b_out; a.outputs = outputs; a.h_n = h_n; a.attn_w = attn_w;
    a.B = B; a.Te = Te; a.H = H; a.nl = n_layers; a.n_frames = n_frames; a.n_pre = n_pre; a.Pd = Pd; a.Po = Po; a.Z = Z; a.S8 = S8;
    hipLaunchKernelGGL(seq2seq_decode_kernel, dim3(B), dim3(DEC_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tg_seq2seq_decode_eval");
}

}  // extern "C"
