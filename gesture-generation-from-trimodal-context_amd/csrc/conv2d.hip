// 2-D convolution as an implicit GEMM on the bf16 matrix cores (Speech2Gesture's audio encoder), and the small element-wise ops of that
// model (row interpolation of make_1d, UnetUp's repeat x 2 + crop + add, first differences, the LSGAN mean-squared terms).
//
// Layout: activations channel-last fp32 (B, H, W, C) -- the input may also be fp16 (the spectrogram as the loader delivers it); weights
// in nn.Conv2d's own layout [Co][Ci][kh][kw], read in place (no packing pass).  Geometry: output (Ho, Wo), stride s in both axes, explicit
// top / left zero padding; bottom / right zeros come from the bounds checks, which is how TF "SAME" puts the odd extra zero there.
//
//   forward  C[m = (b, ho, wo)][n = co]      = sum_{k = (i, j, ci)} x[b, ho s - pt + i, wo s - pl + j, ci] * w[co, ci, i, j] + bias[co]
//   dgrad    C[m = (b, h, w)][n = ci]        = sum_{k = (i, j, co)} dy[b, (h + pt - i) / s, (w + pl - j) / s, co] * w[co, ci, i, j]
//                                              (taps whose offset is not a multiple of s, or that fall outside dy, are zero)
//   wgrad    P_z[m = co][n = (i, j, ci)]     = sum_{r in split z} dy[r, co] * x[gather of (r, i, j, ci)]   (split K, r = (b, ho, wo))
//            dw[co, ci, i, j] (+)= sum_z P_z    (fixed order, fp64: bitwise repeatable whatever the mode)
//
// No im2col buffer: each thread gathers its operand elements straight from the tensor while the 32-deep K slab is staged, splits them
// exactly into three bf16 terms (common.hpp split3_bits, x = hi + mid + lo) and stores the planes to LDS; the product keeps the six partial
// products of weight >= 2^-16 (hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi), each an exact bf16 product accumulated in fp32 by
// v_mfma_f32_16x16x32_bf16 -- the accuracy contract of gemm_split.hip.  Math mode 1 (tg_set_math_mode) uses one round-to-nearest bf16
// term and one MFMA instead.  Workgroup tile 64 x 64, four waves as 2 x 2, wave tile 32 x 32 (2 x 2 MFMA tiles); the next slab's global
// loads are in flight while the current one is multiplied.
#include "operand_split.hpp"

namespace tg {

struct C2Geom {
    int B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo;
};

constexpr int C2_BM = 64, C2_BN = 64, C2_BK = 32, C2_LDK = 40;     // LDS rows of 32 bf16 padded to 80 bytes (16-byte aligned fragment reads)

template <typename TX>
__device__ __forceinline__ float c2_ld(const TX* p) { return (float)*p; }

// n consecutive K values of one LDS row (n = 4 or 8, k0 a multiple of n) -> SPLITS bf16 planes
template <int SPLITS, int NV>
__device__ __forceinline__ void c2_store(const float (&v)[NV], __bf16* dst, long plane) {
    unsigned h[NV], m[NV], l[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        if constexpr (SPLITS == 1) {
            const __bf16 r = (__bf16)v[q];
            h[q] = (unsigned)__builtin_bit_cast(unsigned short, r) << 16;
        } else {
            split3_bits(v[q], h[q], m[q], l[q]);
        }
    }
#pragma unroll
    for (int s = 0; s < SPLITS; ++s) {
        const unsigned* src = s == 0 ? h : (s == 1 ? m : l);
        if constexpr (NV == 4) {
            *reinterpret_cast<u32x2*>(dst + s * plane) = u32x2{pack_hi16(src[0], src[1]), pack_hi16(src[2], src[3])};
        } else {
            *reinterpret_cast<u32x4*>(dst + s * plane) =
                u32x4{pack_hi16(src[0], src[1]), pack_hi16(src[2], src[3]), pack_hi16(src[4], src[5]), pack_hi16(src[6], src[7])};
        }
    }
}

// MODE 0: forward (A = x gather, B = w), MODE 1: input gradient (A = dy gather, B = w), MODE 2: weight-gradient split z = blockIdx.y
// (A = dy^T, B = x gather^T, K range [z r_chunk, (z + 1) r_chunk) of R = B Ho Wo).  M / N / K as in the file comment.
template <int MODE, int SPLITS, typename TX>
__global__ __launch_bounds__(256) void conv2d_mfma_kernel(const C2Geom g, const TX* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ dy, const float* __restrict__ bias, float* __restrict__ out,
                                                          int M, int N, int K, int n_nt, int r_chunk, int accumulate) {
    constexpr int NS = SPLITS;
    __shared__ __attribute__((aligned(16))) __bf16 lds[NS][2][C2_BM][C2_LDK];
    constexpr long PLANE = 2L * C2_BM * C2_LDK;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = (blockIdx.x / n_nt) * C2_BM, n0 = (blockIdx.x % n_nt) * C2_BN;
    const int T = g.kh * g.kw;
    int kbeg = 0, kend = K;
    if constexpr (MODE == 2) {
        kbeg = blockIdx.y * r_chunk;
        kend = min(K, kbeg + r_chunk);
    }

    // ---- fixed per-thread row decodes
    // MODE 0 / 1: rows (t >> 3) + {0, 32} of both operands, K piece 4 (t & 7) .. + 3;  MODE 2: row t & 63, K piece 8 (t >> 6) .. + 7
    int ra_b[2], ra_h[2], ra_w[2];
    bool ra_ok[2], rb_ok[2];
    int rb_n[2];
    if constexpr (MODE != 2) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int m = m0 + (t >> 3) + 32 * q;
            ra_ok[q] = m < M;
            const int mm = ra_ok[q] ? m : 0;
            const int HW = MODE == 0 ? g.Ho * g.Wo : g.H * g.W, Wd = MODE == 0 ? g.Wo : g.W;
            const int b = mm / HW, rem = mm - b * HW, hh = rem / Wd, ww = rem - hh * Wd;
            ra_b[q] = b;
            ra_h[q] = MODE == 0 ? hh * g.s - g.pt : hh + g.pt;
            ra_w[q] = MODE == 0 ? ww * g.s - g.pl : ww + g.pl;
            const int n = n0 + (t >> 3) + 32 * q;
            rb_ok[q] = n < N;
            rb_n[q] = rb_ok[q] ? n : 0;
        }
    }
    int wg_co = 0, wg_i = 0, wg_j = 0, wg_ci = 0;
    bool wg_aok = false, wg_bok = false;
    if constexpr (MODE == 2) {
        const int row = t & 63;
        wg_co = m0 + row;
        wg_aok = wg_co < M;
        const int n = n0 + row;
        wg_bok = n < N;
        const int nn = wg_bok ? n : 0;
        const int tap = nn / g.Ci;
        wg_ci = nn - tap * g.Ci;
        wg_i = tap / g.kw;
        wg_j = tap - wg_i * g.kw;
    }

    float va[8], vb[8];                                         // this slab's operand elements (MODE 0 / 1: [row q][4 K], MODE 2: 8 K)

    auto load = [&](int k0) {
        if constexpr (MODE != 2) {
            const int kp = k0 + 4 * (t & 7);
            const int Cred = MODE == 0 ? g.Ci : g.Co;            // K = (tap, channel), channel fastest
            int tap = kp / Cred, c = kp - tap * Cred;
            int i = tap / g.kw, j = tap - i * g.kw;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool kok = kp + u < kend;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float a = 0.f, bv = 0.f;
                    if (kok && ra_ok[q]) {
                        if constexpr (MODE == 0) {
                            const int h = ra_h[q] + i, ww = ra_w[q] + j;
                            if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W)
                                a = c2_ld(x + (((long)ra_b[q] * g.H + h) * g.W + ww) * g.Ci + c);
                        } else {
                            const int hn = ra_h[q] - i, wn_ = ra_w[q] - j;
                            if (hn >= 0 && wn_ >= 0 && hn % g.s == 0 && wn_ % g.s == 0) {
                                const int ho = hn / g.s, wo = wn_ / g.s;
                                if (ho < g.Ho && wo < g.Wo) a = dy[(((long)ra_b[q] * g.Ho + ho) * g.Wo + wo) * g.Co + c];
                            }
                        }
                    }
                    if (kok && rb_ok[q]) {
                        if constexpr (MODE == 0) bv = w[((long)rb_n[q] * g.Ci + c) * T + tap];
                        else bv = w[((long)c * g.Ci + rb_n[q]) * T + tap];
                    }
                    va[4 * q + u] = a;
                    vb[4 * q + u] = bv;
                }
                if (++c == Cred) {
                    c = 0;
                    ++tap;
                    if (++j == g.kw) { j = 0; ++i; }
                }
            }
        } else {
            const int r0 = k0 + 8 * (t >> 6);
            const int HW = g.Ho * g.Wo;
            int b = r0 / HW, rem = r0 - b * HW, ho = rem / g.Wo, wo = rem - ho * g.Wo;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = r0 + u;
                float a = 0.f, bv = 0.f;
                if (r < kend) {
                    if (wg_aok) a = dy[(long)r * g.Co + wg_co];
                    if (wg_bok) {
                        const int h = ho * g.s - g.pt + wg_i, ww = wo * g.s - g.pl + wg_j;
                        if ((unsigned)h < (unsigned)g.H && (unsigned)ww < (unsigned)g.W)
                            bv = c2_ld(x + (((long)b * g.H + h) * g.W + ww) * g.Ci + wg_ci);
                    }
                }
                va[u] = a;
                vb[u] = bv;
                if (++wo == g.Wo) { wo = 0; if (++ho == g.Ho) { ho = 0; ++b; } }
            }
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += C2_BK) {
        __syncthreads();                                          // the previous slab's fragment reads are done
        if constexpr (MODE != 2) {
            const int kc = 4 * (t & 7);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int row = (t >> 3) + 32 * q;
                const float pa[4] = {va[4 * q], va[4 * q + 1], va[4 * q + 2], va[4 * q + 3]};
                const float pb[4] = {vb[4 * q], vb[4 * q + 1], vb[4 * q + 2], vb[4 * q + 3]};
                c2_store<SPLITS, 4>(pa, &lds[0][0][row][kc], PLANE);
                c2_store<SPLITS, 4>(pb, &lds[0][1][row][kc], PLANE);
            }
        } else {
            const int row = t & 63, kc = 8 * (t >> 6);
            c2_store<SPLITS, 8>(va, &lds[0][0][row][kc], PLANE);
            c2_store<SPLITS, 8>(vb, &lds[0][1][row][kc], PLANE);
        }
        __syncthreads();
        if (k0 + C2_BK < kend) load(k0 + C2_BK);                   // in flight during the MFMAs below
        bf16x8 fa[NS][2], fb[NS][2];
        const int fr = lane & 15, fk = 8 * (lane >> 4);
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[s][i] = *reinterpret_cast<const bf16x8*>(&lds[s][0][wm * 32 + i * 16 + fr][fk]);
                fb[s][i] = *reinterpret_cast<const bf16x8*>(&lds[s][1][wn * 32 + i * 16 + fr][fk]);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x4 c = acc[i][j];
                if constexpr (SPLITS == 3) {                      // smallest terms first
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[2][i], fb[0][j], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][i], fb[2][j], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][i], fb[1][j], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[1][i], fb[0][j], c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][i], fb[1][j], c, 0, 0, 0);
                }
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[0][i], fb[0][j], c, 0, 0, 0);
                acc[i][j] = c;
            }
    }

    // ---- epilogue: lane holds C[row 4 (lane >> 4) + r][col lane & 15] of each 16 x 16 tile
    float* __restrict__ dst = out;
    if constexpr (MODE == 2) dst = out + (long)blockIdx.y * M * N;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 32 + j * 16 + (lane & 15);
            if (col >= N) continue;
            const float bb = (MODE == 0 && bias) ? bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 32 + i * 16 + 4 * (lane >> 4) + r;
                if (row >= M) continue;
                float* p = dst + (long)row * N + col;
                const float v = acc[i][j][r] + bb;
                *p = (MODE == 1 && accumulate) ? *p + v : v;
            }
        }
}

// dw[co, ci, i, j] (+)= sum_z P_z[co][(i kw + j) Ci + ci], z = 0 .. splits - 1 in order, in fp64
__global__ __launch_bounds__(256) void conv2d_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int Co, int Ci, int T, float* __restrict__ dw,
                                                                  int accumulate) {
    const long total = (long)Co * Ci * T, MN = total;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long co = e / ((long)Ci * T);
        const int rem = (int)(e - co * Ci * T), ci = rem / T, tap = rem - ci * T;
        const long n = co * ((long)T * Ci) + (long)tap * Ci + ci;
        double s = 0.0;
        for (int z = 0; z < splits; ++z) s += (double)ws[(long)z * MN + n];
        dw[e] = accumulate ? (float)((double)dw[e] + s) : (float)s;
    }
}

// ---- small ops of the Speech2Gesture generator / discriminator ---------------------------------------------------------------------

// torch's bilinear source row (align_corners=False, size given): src = max(0, (t + 0.5) Hin / Hout - 0.5), rows h0 / h1, weight of h1.
// In integers, src = ((2 t + 1) Hin - Hout) / (2 Hout): the row is exact and the weight is rounded once.  (In fp32 the weight carries the
// rounding of Hin / Hout times src, 1.7e-6 of the output at 34 -> 14.)
__device__ __forceinline__ void interp_src(int t, int Hin, int Hout, int& h0, int& h1, float& l1) {
    const long den = 2L * Hout;
    long num = (2L * t + 1) * Hin - Hout;
    num = num < 0 ? 0 : num;
    const long q = num / den;
    h0 = q > Hin - 1 ? Hin - 1 : (int)q;
    h1 = h0 + 1 < Hin ? h0 + 1 : h0;
    l1 = (float)(num - q * den) / (float)den;
}

// y[b, t, c] = (1 - l) x[b, h0, col, c] + l x[b, h1, col, c]     x (B, Hin, Win, C), y (B, Hout, C)
__global__ __launch_bounds__(256) void rows_interp_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int Hin, int Wd, int col, int C, int Hout) {
    const long total = (long)B * Hout * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long bt = e / C;
        const int tt = (int)(bt % Hout), b = (int)(bt / Hout);
        int h0, h1;
        float l1;
        interp_src(tt, Hin, Hout, h0, h1, l1);
        const float a = x[(((long)b * Hin + h0) * Wd + col) * C + c], d = x[(((long)b * Hin + h1) * Wd + col) * C + c];
        y[e] = (1.f - l1) * a + l1 * d;
    }
}

// dx[b, h, w, c] = (w == col) sum_t [h0(t) == h] (1 - l(t)) dy[b, t, c] + [h1(t) == h] l(t) dy[b, t, c]   (written, zeros off column col)
__global__ __launch_bounds__(256) void rows_interp_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int Hin, int Wd, int col, int C, int Hout) {
    const long total = (long)B * Hin * Wd * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        long r = e / C;
        const int wcol = (int)(r % Wd);
        r /= Wd;
        const int h = (int)(r % Hin), b = (int)(r / Hin);
        float s = 0.f;
        if (wcol == col)
            for (int tt = 0; tt < Hout; ++tt) {
                int h0, h1;
                float l1;
                interp_src(tt, Hin, Hout, h0, h1, l1);
                const float g = dy[((long)b * Hout + tt) * C + c];
                if (h0 == h) s += (1.f - l1) * g;
                if (h1 == h) s += l1 * g;
            }
        dx[e] = s;
    }
}

// y[b, t, c] = x[b, t / 2, c] + skip[b, t, c], t < Ls
__global__ __launch_bounds__(256) void up_add_kernel(const float* __restrict__ x, const float* __restrict__ skip, float* __restrict__ y, int B, int Lx, int Ls, int C) {
    const long total = (long)B * Ls * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long bt = e / C;
        const int tt = (int)(bt % Ls), b = (int)(bt / Ls);
        y[e] = x[((long)b * Lx + tt / 2) * C + c] + skip[e];
    }
}

// dx[b, l, c] (+)= dy[b, 2l, c] + dy[b, 2l + 1, c]   (rows past Ls contribute nothing)
__global__ __launch_bounds__(256) void up_add_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int Lx, int Ls, int C, int accumulate) {
    const long total = (long)B * Lx * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long bl = e / C;
        const int l = (int)(bl % Lx), b = (int)(bl / Lx);
        float s = 0.f;
        if (2 * l < Ls) s += dy[((long)b * Ls + 2 * l) * C + c];
        if (2 * l + 1 < Ls) s += dy[((long)b * Ls + 2 * l + 1) * C + c];
        dx[e] = accumulate ? dx[e] + s : s;
    }
}

// y[b, t, c] = x[b, t + 1, c] - x[b, t, c], t < T - 1
__global__ __launch_bounds__(256) void diff_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int T, int C) {
    const long total = (long)B * (T - 1) * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long bt = e / C;
        const int tt = (int)(bt % (T - 1)), b = (int)(bt / (T - 1));
        const long i = ((long)b * T + tt) * C + c;
        y[e] = x[i + C] - x[i];
    }
}

// dx[b, t, c] (+)= dy[b, t - 1, c] - dy[b, t, c]   (terms outside [0, T - 1) are zero)
__global__ __launch_bounds__(256) void diff_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int T, int C, int accumulate) {
    const long total = (long)B * T * C;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const long bt = e / C;
        const int tt = (int)(bt % T), b = (int)(bt / T);
        float s = 0.f;
        if (tt > 0) s += dy[((long)b * (T - 1) + tt - 1) * C + c];
        if (tt < T - 1) s -= dy[((long)b * (T - 1) + tt) * C + c];
        dx[e] = accumulate ? dx[e] + s : s;
    }
}

// loss[0] = mean((x - target)^2) (fp64 sums in thread order: one workgroup, bitwise repeatable); dx = scale 2 (x - target) / n
__global__ __launch_bounds__(256) void mse_const_kernel(const float* __restrict__ x, long n, float target, float scale, float* __restrict__ loss,
                                                        float* __restrict__ dx) {
    __shared__ double part[256];
    double s = 0.0;
    const float g = 2.f * scale / (float)n;
    for (long i = threadIdx.x; i < n; i += 256) {
        const float d = x[i] - target;
        s += (double)d * (double)d;
        if (dx) dx[i] = g * d;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot += part[i];
        loss[0] = (float)(tot / (double)n);
    }
}

// d[i] = sign(a[i] - b[i]) / n   (the gradient of mean |a - b|; 0 where a == b, as torch's L1Loss)
__global__ __launch_bounds__(256) void l1_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ d, long n) {
    const float inv = 1.f / (float)n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float e = a[i] - b[i];
        d[i] = e > 0.f ? inv : (e < 0.f ? -inv : 0.f);
    }
}

}  // namespace tg

using namespace tg;

extern "C" int tg_get_math_mode(void);

// geometry check shared by the three conv entry points: every size positive, stride 1 or 2, pads inside the kernel, the output inside the
// padded input, every product index within int32
static int c2_check(const char* what, int B, int H, int W, int Ci, int Co, int kh, int kw, int s, int pt, int pl, int Ho, int Wo, C2Geom& g) {
    TG_REQUIRE(B > 0 && H > 0 && W > 0 && Ci > 0 && Co > 0 && kh > 0 && kw > 0 && kh <= 8 && kw <= 8 && (s == 1 || s == 2) && Ho > 0 && Wo > 0,
               "%s: bad geometry (sizes > 0, kernel <= 8 x 8, stride 1 or 2)", what);
    TG_REQUIRE(pt >= 0 && pl >= 0 && pt < kh && pl < kw, "%s: pads (%d, %d) must lie in [0, kernel)", what, pt, pl);
    const int64_t pb = (int64_t)(Ho - 1) * s + kh - pt - H, pr = (int64_t)(Wo - 1) * s + kw - pl - W;   // implied bottom / right zeros
    TG_REQUIRE(pb < kh && pr < kw && (int64_t)(Ho - 1) * s - pt < H && (int64_t)(Wo - 1) * s - pl < W,
               "%s: output %d x %d does not fit a %d x %d input (k %d x %d, stride %d, pads %d, %d)", what, Ho, Wo, H, W, kh, kw, s, pt, pl);
    const int64_t lim = (int64_t)1 << 30;
    TG_REQUIRE((int64_t)B * H * W * Ci < lim * 2 && (int64_t)B * Ho * Wo * Co < lim * 2 && (int64_t)B * H * W < lim && (int64_t)B * Ho * Wo < lim &&
                   (int64_t)kh * kw * Ci < lim && (int64_t)kh * kw * Co < lim,
               "%s: tensor too large for 32-bit row indices", what);
    g = C2Geom{B, H, W, Ci, Co, kh, kw, s, pt, pl, Ho, Wo};
    return 0;
}

// split-K plan of the weight gradient: enough workgroups to cover the CUs about four times, at least 256 rows per split
static void c2_wgrad_plan(const C2Geom& g, int& splits, int& r_chunk) {
    const int64_t R = (int64_t)g.B * g.Ho * g.Wo;
    const int64_t tiles = (int64_t)cdiv(g.Co, C2_BM) * cdiv((int64_t)g.kh * g.kw * g.Ci, C2_BN);
    int64_t sp = (1024 + tiles - 1) / tiles;
    const int64_t by_rows = (R + 255) / 256;
    if (sp > by_rows) sp = by_rows;
    if (sp > 256) sp = 256;
    if (sp < 1) sp = 1;
    int64_t ch = (R + sp - 1) / sp;
    ch = (ch + C2_BK - 1) / C2_BK * C2_BK;
    r_chunk = (int)ch;
    splits = (int)((R + ch - 1) / ch);
}

extern "C" int tg_conv2d_fwd(const void* x, int32_t x_half, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W, int32_t Ci,
                             int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* stream) {
    TG_REQUIRE(x && w && y && (x_half == 0 || x_half == 1), "tg_conv2d_fwd: bad arguments");
    C2Geom g;
    if (int e = c2_check("tg_conv2d_fwd", B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo, g)) return e;
    const int M = B * Ho * Wo, N = Co, K = kh * kw * Ci;
    const int n_nt = cdiv(N, C2_BN);
    const dim3 grid((unsigned)((int64_t)cdiv(M, C2_BM) * n_nt));
    hipStream_t s = (hipStream_t)stream;
    const bool one = tg_get_math_mode() == 1;
#define TG_C2F(SP, TX) hipLaunchKernelGGL((conv2d_mfma_kernel<0, SP, TX>), grid, dim3(256), 0, s, g, (const TX*)x, w, (const float*)nullptr, bias, y, M, N, K, n_nt, 0, 0)
    if (x_half) { if (one) TG_C2F(1, _Float16); else TG_C2F(3, _Float16); }
    else { if (one) TG_C2F(1, float); else TG_C2F(3, float); }
#undef TG_C2F
    return check_launch("tg_conv2d_fwd");
}

extern "C" int tg_conv2d_dgrad(const float* dy, const float* w, float* dx, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                               int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* stream) {
    TG_REQUIRE(dy && w && dx && (accumulate == 0 || accumulate == 1), "tg_conv2d_dgrad: bad arguments");
    C2Geom g;
    if (int e = c2_check("tg_conv2d_dgrad", B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo, g)) return e;
    const int M = B * H * W, N = Ci, K = kh * kw * Co;
    const int n_nt = cdiv(N, C2_BN);
    const dim3 grid((unsigned)((int64_t)cdiv(M, C2_BM) * n_nt));
    hipStream_t s = (hipStream_t)stream;
#define TG_C2D(SP) hipLaunchKernelGGL((conv2d_mfma_kernel<1, SP, float>), grid, dim3(256), 0, s, g, (const float*)nullptr, w, dy, (const float*)nullptr, dx, M, N, K, n_nt, 0, accumulate)
    if (tg_get_math_mode() == 1) TG_C2D(1); else TG_C2D(3);
#undef TG_C2D
    return check_launch("tg_conv2d_dgrad");
}

extern "C" int tg_conv2d_wgrad_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top,
                                        int32_t pad_left, int32_t Ho, int32_t Wo, int64_t* bytes) {
    TG_REQUIRE(bytes, "tg_conv2d_wgrad_ws_bytes: bad arguments");
    C2Geom g;
    if (int e = c2_check("tg_conv2d_wgrad_ws_bytes", B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo, g)) return e;
    int splits, r_chunk;
    c2_wgrad_plan(g, splits, r_chunk);
    *bytes = (int64_t)splits * Co * kh * kw * Ci * (int64_t)sizeof(float);
    return 0;
}

extern "C" int tg_conv2d_wgrad(const float* dy, const void* x, int32_t x_half, float* dw, int32_t accumulate, float* ws, int64_t ws_bytes, int32_t B, int32_t H,
                               int32_t W, int32_t Ci, int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho,
                               int32_t Wo, void* stream) {
    TG_REQUIRE(dy && x && dw && ws && (x_half == 0 || x_half == 1) && (accumulate == 0 || accumulate == 1), "tg_conv2d_wgrad: bad arguments");
    C2Geom g;
    if (int e = c2_check("tg_conv2d_wgrad", B, H, W, Ci, Co, kh, kw, stride, pad_top, pad_left, Ho, Wo, g)) return e;
    int splits, r_chunk;
    c2_wgrad_plan(g, splits, r_chunk);
    const int M = Co, N = kh * kw * Ci, K = B * Ho * Wo;
    TG_REQUIRE(ws_bytes >= (int64_t)splits * M * N * (int64_t)sizeof(float), "tg_conv2d_wgrad: workspace of %lld bytes, %lld needed (tg_conv2d_wgrad_ws_bytes)",
               (long long)ws_bytes, (long long)((int64_t)splits * M * N * 4));
    const int n_nt = cdiv(N, C2_BN);
    const dim3 grid((unsigned)((int64_t)cdiv(M, C2_BM) * n_nt), (unsigned)splits);
    hipStream_t s = (hipStream_t)stream;
    const bool one = tg_get_math_mode() == 1;
#define TG_C2W(SP, TX) hipLaunchKernelGGL((conv2d_mfma_kernel<2, SP, TX>), grid, dim3(256), 0, s, g, (const TX*)x, (const float*)nullptr, dy, (const float*)nullptr, ws, M, N, K, n_nt, r_chunk, 0)
    if (x_half) { if (one) TG_C2W(1, _Float16); else TG_C2W(3, _Float16); }
    else { if (one) TG_C2W(1, float); else TG_C2W(3, float); }
#undef TG_C2W
    if (check_launch("tg_conv2d_wgrad")) return 1;
    hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3(ew_grid((int64_t)M * N, 256, 1)), dim3(256), 0, s, ws, splits, Co, Ci, kh * kw, dw, accumulate);
    return check_launch("tg_conv2d_wgrad(reduce)");
}

extern "C" int tg_s2g_rows_interp(const float* x, float* y, int32_t B, int32_t Hin, int32_t Win, int32_t col, int32_t C, int32_t Hout, void* stream) {
    TG_REQUIRE(x && y && B > 0 && Hin > 0 && Win > 0 && col >= 0 && col < Win && C > 0 && Hout > 0, "tg_s2g_rows_interp: bad arguments");
    hipLaunchKernelGGL(rows_interp_kernel, dim3(ew_grid((int64_t)B * Hout * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, x, y, B, Hin, Win, col, C, Hout);
    return check_launch("tg_s2g_rows_interp");
}

extern "C" int tg_s2g_rows_interp_bwd(const float* dy, float* dx, int32_t B, int32_t Hin, int32_t Win, int32_t col, int32_t C, int32_t Hout, void* stream) {
    TG_REQUIRE(dy && dx && B > 0 && Hin > 0 && Win > 0 && col >= 0 && col < Win && C > 0 && Hout > 0, "tg_s2g_rows_interp_bwd: bad arguments");
    hipLaunchKernelGGL(rows_interp_bwd_kernel, dim3(ew_grid((int64_t)B * Hin * Win * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, dy, dx, B, Hin, Win, col,
                       C, Hout);
    return check_launch("tg_s2g_rows_interp_bwd");
}

extern "C" int tg_s2g_up_add(const float* x, const float* skip, float* y, int32_t B, int32_t Lx, int32_t Ls, int32_t C, void* stream) {
    TG_REQUIRE(x && skip && y && B > 0 && Lx > 0 && Ls > 0 && Ls <= 2 * Lx && C > 0, "tg_s2g_up_add: bad arguments (Ls <= 2 Lx)");
    hipLaunchKernelGGL(up_add_kernel, dim3(ew_grid((int64_t)B * Ls * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, x, skip, y, B, Lx, Ls, C);
    return check_launch("tg_s2g_up_add");
}

extern "C" int tg_s2g_up_add_bwd(const float* dy, float* dx, int32_t B, int32_t Lx, int32_t Ls, int32_t C, int32_t accumulate, void* stream) {
    TG_REQUIRE(dy && dx && B > 0 && Lx > 0 && Ls > 0 && Ls <= 2 * Lx && C > 0 && (accumulate == 0 || accumulate == 1), "tg_s2g_up_add_bwd: bad arguments");
    hipLaunchKernelGGL(up_add_bwd_kernel, dim3(ew_grid((int64_t)B * Lx * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, dy, dx, B, Lx, Ls, C, accumulate);
    return check_launch("tg_s2g_up_add_bwd");
}

extern "C" int tg_s2g_diff(const float* x, float* y, int32_t B, int32_t T, int32_t C, void* stream) {
    TG_REQUIRE(x && y && B > 0 && T > 1 && C > 0, "tg_s2g_diff: bad arguments (T >= 2)");
    hipLaunchKernelGGL(diff_kernel, dim3(ew_grid((int64_t)B * (T - 1) * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, x, y, B, T, C);
    return check_launch("tg_s2g_diff");
}

extern "C" int tg_s2g_diff_bwd(const float* dy, float* dx, int32_t B, int32_t T, int32_t C, int32_t accumulate, void* stream) {
    TG_REQUIRE(dy && dx && B > 0 && T > 1 && C > 0 && (accumulate == 0 || accumulate == 1), "tg_s2g_diff_bwd: bad arguments (T >= 2)");
    hipLaunchKernelGGL(diff_bwd_kernel, dim3(ew_grid((int64_t)B * T * C, 256, 1)), dim3(256), 0, (hipStream_t)stream, dy, dx, B, T, C, accumulate);
    return check_launch("tg_s2g_diff_bwd");
}

extern "C" int tg_s2g_mse_const(const float* x, int64_t n, float target, float scale, float* loss, float* dx, void* stream) {
    TG_REQUIRE(x && loss && n > 0 && n <= ((int64_t)1 << 30), "tg_s2g_mse_const: bad arguments");
    hipLaunchKernelGGL(mse_const_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, (long)n, target, scale, loss, dx);
    return check_launch("tg_s2g_mse_const");
}

extern "C" int tg_s2g_l1_grad(const float* a, const float* b, float* d, int64_t n, void* stream) {
    TG_REQUIRE(a && b && d && n > 0, "tg_s2g_l1_grad: bad arguments");
    hipLaunchKernelGGL(l1_grad_kernel, dim3(ew_grid(n, 256, 4)), dim3(256), 0, (hipStream_t)stream, a, b, d, (long)n);
    return check_launch("tg_s2g_l1_grad");
}
