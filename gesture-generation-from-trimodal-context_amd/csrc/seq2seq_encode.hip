// The eval-mode recurrence of one GRU layer with per-row lengths (the Seq2Seq text encoder, model/seq2seq_net.py:14-56) in ONE launch, one
// workgroup per (batch row, direction): the contract of tg_gru_seq_forward without a tape.
//
// gru_seq.hip runs one launch per time step; at the one to four rows of streaming synthesis that chain of T launches per layer is what an
// encoder forward spends its time in, and its length follows the longest row, which a captured graph cannot have.  Without a tape nothing
// couples one row to another or one direction to the other, so a workgroup owns its (row, direction) for all of the row's len steps: the
// state lives in LDS, W_hh [3H][H] is re-read from L2 every step (480 KB per direction at H = 200), and no workgroup ever waits on another --
// no spin, no flag, no atomic (the structure of seq2seq_decode.hip, not the exchange protocol of gru_vec.hip).  Per step, at position
// t = s (forward) or len - 1 - s (reverse, which therefore starts at the row's last valid position):
//
//   gh = W_hh h;  (r, z, n, h) = gru_cell_fwd(gi[dir][b][t], gh, b_hh, h)  (gru_step.hpp);  y[b][t][dir H ..] = h
//
// then y[b][t >= len] = exact zeros, written here so that a static buffer needs no fill pass, and h_n[dir][b] = the state after the last
// step -- the very value stored at y[b][len - 1][:H] / y[b][0][H:].  The product is a matrix-vector product in fp32 FMA: a quarter wave per
// output row, ENC_RU rows of a quarter in flight at once, float4 lanes over K (W_hh rows are 16-byte aligned: H % 4 == 0), the 16 partial sums
// meet in a four-step exchange.  Every sum runs in an order fixed by H alone: a row's result does not depend on B, on the row's place in
// the batch or on T, and two runs are bit-identical.  A lengths entry outside [1, T] skips the row (y = 0, h_n = h0) and sets *flag; nothing
// outside the row is read or written.
#include "common.hpp"
#include "gru_step.hpp"

namespace tg {

constexpr int ENC_THREADS = 512, ENC_QUARTERS = ENC_THREADS / 16, ENC_RU = 4, ENC_JU = 4;
constexpr int ENC_MAX_T = 128, ENC_MAX_H = 320;
#define ENC_ENVELOPE "D in {1, 2}, B >= 1, 1 <= T <= 128, H %% 4 == 0, 8 <= H <= 320"

inline bool enc_in_envelope(int64_t B, int64_t T, int64_t H, int64_t D) {
    return (D == 1 || D == 2) && B >= 1 && B <= 0x7fffffffLL && T >= 1 && T <= ENC_MAX_T && H >= 8 && H <= ENC_MAX_H && H % 4 == 0;
}

// store(r, W[r, :4 nj4] . x) for r < rows.  W rows are 4 nj4 floats long and 16-byte aligned; x lies in LDS.
template <typename F>
__device__ __forceinline__ void enc_matvec(const float* __restrict__ W, int rows, int nj4, const float* x, int quarter, int l16, F store) {
    const int K = 4 * nj4;
    for (int r0 = quarter * ENC_RU; r0 < rows; r0 += ENC_QUARTERS * ENC_RU) {
        const float* wr[ENC_RU];
        float acc[ENC_RU];
#pragma unroll
        for (int u = 0; u < ENC_RU; ++u) {
            const int r = r0 + u < rows ? r0 + u : rows - 1;          // a row past the end repeats the last one and is not stored
            wr[u] = W + (long)r * K;
            acc[u] = 0.f;
        }
        for (int jb = 0; jb < nj4; jb += 16 * ENC_JU) {
            f32x4 w[ENC_RU][ENC_JU];
#pragma unroll
            for (int u = 0; u < ENC_RU; ++u)
#pragma unroll
                for (int v = 0; v < ENC_JU; ++v) {
                    const int j = jb + 16 * v + l16;
                    w[u][v] = j < nj4 ? *reinterpret_cast<const f32x4*>(wr[u] + 4 * j) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
            for (int v = 0; v < ENC_JU; ++v) {
                const int j = jb + 16 * v + l16;
                if (j < nj4) {
                    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + 4 * j);
#pragma unroll
                    for (int u = 0; u < ENC_RU; ++u)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[u] = fmaf(w[u][v][c], xv[c], acc[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < ENC_RU; ++u) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o, 64);
            if (l16 == 0 && r0 + u < rows) store(r0 + u, acc[u]);
        }
    }
}

__global__ __launch_bounds__(ENC_THREADS) void seq2seq_encode_kernel(const float* __restrict__ gi, const float* __restrict__ whh0,
                                                                     const float* __restrict__ whh1, const float* __restrict__ bhh0,
                                                                     const float* __restrict__ bhh1, const float* __restrict__ h0,
                                                                     const long long* __restrict__ lengths, float* __restrict__ Y,
                                                                     float* __restrict__ hn_out, int* __restrict__ flag, int B, int T, int H, int D) {
    __shared__ __attribute__((aligned(16))) float s_h[ENC_MAX_H], s_gh[3 * ENC_MAX_H];
    const int tid = threadIdx.x, b = blockIdx.x, dir = blockIdx.y;
    const int quarter = tid >> 4, l16 = tid & 15, nj4 = H >> 2;
    const float* __restrict__ whh = dir ? whh1 : whh0;
    const float* __restrict__ bhh = dir ? bhh1 : bhh0;
    const long DH = (long)D * H;
    float* __restrict__ yb = Y + (long)b * T * DH + (long)dir * H;                     // this direction's H columns of the row's T positions
    const float* __restrict__ gb = gi + ((long)dir * B + b) * (long)T * (3 * H);
    int len = T;
    bool skipped = false;
    if (lengths) {
        const long long v = lengths[b];
        skipped = v < 1 || v > T;
        len = skipped ? 0 : (int)v;
    }
    const bool own = tid < H;
    float bh_r = 0.f, bh_z = 0.f, bh_n = 0.f, hp = 0.f;
    if (own) {
        bh_r = bhh[tid]; bh_z = bhh[H + tid]; bh_n = bhh[2 * H + tid];
        hp = h0 ? h0[((long)dir * B + b) * H + tid] : 0.f;
        s_h[tid] = hp;
    }
    __syncthreads();
    for (int s = 0; s < len; ++s) {
        const int t = dir ? len - 1 - s : s;
        // the gate epilogue's operands go out before the product
        float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f;
        if (own) {
            const float* gp = gb + (long)t * (3 * H);
            gi_r = gp[tid]; gi_z = gp[H + tid]; gi_n = gp[2 * H + tid];
        }
        enc_matvec(whh, 3 * H, nj4, s_h, quarter, l16, [&](int r, float v) { s_gh[r] = v; });
        __syncthreads();
        if (own) {
            const float gh[3] = {s_gh[tid], s_gh[H + tid], s_gh[2 * H + tid]};
            const GruCell c = gru_cell_fwd(gi_r, gi_z, gi_n, gh, bh_r, bh_z, bh_n, hp);
            hp = c.h;
            s_h[tid] = c.h;
            yb[(long)t * DH + tid] = c.h;
        }
        __syncthreads();
    }
    // padded positions: exact zeros; the final state: the last step's value (h0 for a skipped row)
    for (int i = tid; i < (T - len) * H; i += ENC_THREADS) {
        const int t = len + i / H, j = i - (i / H) * H;
        yb[(long)t * DH + j] = 0.f;
    }
    if (own) hn_out[((long)dir * B + b) * H + tid] = hp;
    if (skipped && flag && dir == 0 && tid == 0) *flag = 1;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_seq2seq_encode_supported(int32_t B, int32_t T, int32_t H, int32_t D, int32_t* supported) {
    TG_REQUIRE(supported, "tg_seq2seq_encode_supported: null pointer");
    TG_REQUIRE(B > 0 && T > 0 && H > 0 && D > 0, "tg_seq2seq_encode_supported: sizes must be positive (B=%d T=%d H=%d D=%d)", B, T, H, D);
    *supported = enc_in_envelope(B, T, H, D) ? 1 : 0;
    return 0;
}

int tg_seq2seq_encode_eval(const float* gi, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev,
                           const float* h0, const void* lengths, float* y, float* h_n, int32_t* flag, int32_t B, int32_t T, int32_t H, int32_t D,
                           void* stream) {
    TG_REQUIRE(enc_in_envelope(B, T, H, D), "tg_seq2seq_encode_eval: outside the envelope " ENC_ENVELOPE " (B=%d T=%d H=%d D=%d)", B, T, H, D);
    TG_REQUIRE(gi && w_hh_fwd && b_hh_fwd && y && h_n && (D == 1 || (w_hh_rev && b_hh_rev)), "tg_seq2seq_encode_eval: null pointer");
    TG_REQUIRE(aligned16(w_hh_fwd) && aligned16(w_hh_rev), "tg_seq2seq_encode_eval: w_hh must be 16-byte aligned");
    TG_REQUIRE(!lengths || (reinterpret_cast<uintptr_t>(lengths) & 7u) == 0, "tg_seq2seq_encode_eval: lengths must be 8-byte aligned (int64)");
    hipLaunchKernelGGL(seq2seq_encode_kernel, dim3(B, D), dim3(ENC_THREADS), 0, (hipStream_t)stream, gi, w_hh_fwd, D == 2 ? w_hh_rev : w_hh_fwd,
                       b_hh_fwd, D == 2 ? b_hh_rev : b_hh_fwd, h0, (const long long*)lengths, y, h_n, (int*)flag, B, T, H, D);
    return check_launch("tg_seq2seq_encode_eval");
}

}  // extern "C"
