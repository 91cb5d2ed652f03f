// BatchNorm1d (train + eval), channel-last [rows][C].  HBM-bound streaming kernels: coalesced 16-byte accesses,
// per-thread fp64 partial sums, one LDS reduction per workgroup, one fp64 atomic per (workgroup, channel).
// Statistics of "groups" stacked reference forward calls are kept apart (each call normalises with its own batch).
// The arithmetic -- moments, element formulas, the 16-byte loops, the LDS fold -- is csrc/bn_math.hpp; this file is the kernels' data movement.
#include "bn_math.hpp"

namespace tg {

// ---- the streaming chain: zero | reduce | finalize | apply forward, zero | reduce | apply backward.
// Sums of statistics group blockIdx.y into ws [groups][2][C] doubles.  BWD false: (sum x, sum x^2); true: (sum dz, sum dz xhat) with
// dz = dy act'(z) and the group's statistics at mean / rstd + g C (tg_bn_backward: one group)
template <bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy, int rows_per_group, int C,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                        double* __restrict__ ws) {
    __shared__ double sh[2][256];
    const int g = blockIdx.y;
    const int rpi = 256 / C;                 // rows per iteration of this workgroup (C <= 256)
    const int c = threadIdx.x % C, rsub = threadIdx.x / C;
    const long base = (long)g * rows_per_group * C;
    double s = 0.0, ss = 0.0;
    if (rsub < rpi) {
        float mu = 0.f, rs = 0.f, ga = 0.f, be = 0.f;
        if constexpr (BWD) { mu = mean[g * C + c]; rs = rstd[g * C + c]; ga = gamma[c]; be = beta[c]; }
        for (long r = (long)blockIdx.x * rpi + rsub; r < rows_per_group; r += (long)gridDim.x * rpi) {
            const float v = x[base + r * C + c];
            if constexpr (BWD) {
                float xh, dz;
                bn_bwd_element(v, dy[base + r * C + c], mu, rs, ga, be, slope, xh, dz);
                s += dz;
                ss += (double)dz * xh;
            } else {
                s += v;
                ss += (double)v * v;
            }
        }
    }
    sh[0][threadIdx.x] = s;
    sh[1][threadIdx.x] = ss;
    __syncthreads();
    if (threadIdx.x < C) {
        double a = 0.0, b = 0.0;
        for (int q = 0; q < rpi; ++q) { a += sh[0][q * C + c]; b += sh[1][q * C + c]; }
        atomicAdd(&ws[((long)g * 2 + 0) * C + c], a);
        atomicAdd(&ws[((long)g * 2 + 1) * C + c], b);
    }
}

// 16-byte version (C % 4 == 0, C divides 1024): four independent 16-byte loads in flight per thread -- the scalar kernel above has one
// 4-byte load in flight per thread and ran the audio encoder's 21 MB BatchNorm at 0.75 TB/s.
template <bool BWD>
__global__ __launch_bounds__(256) void bn_reduce_vec_kernel(const float* __restrict__ x, const float* __restrict__ dy, long rows_per_group, int C,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                            double* __restrict__ ws) {
    __shared__ double sh[2][256];
    const int g = blockIdx.y;
    const long total4 = rows_per_group * C / 4;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    const int c0 = (int)((i0 * 4) % C);
    bn_lds_zero(sh[0], sh[1], C);
    BnCh ch = {};
    if constexpr (BWD) ch = bn_channels(mean + g * C, rstd + g * C, gamma, beta, c0);
    double s[4], ss[4];
    bn_accumulate<BWD>(reinterpret_cast<const f32x4*>(x) + g * total4, BWD ? reinterpret_cast<const f32x4*>(dy) + g * total4 : nullptr, ch, slope, i0, step, total4, s, ss);
    bn_lds_fold(s, ss, sh[0], sh[1], c0);
    __syncthreads();
    if ((int)threadIdx.x < C) {
        atomicAdd(&ws[((long)g * 2 + 0) * C + threadIdx.x], sh[0][threadIdx.x]);
        atomicAdd(&ws[((long)g * 2 + 1) * C + threadIdx.x], sh[1][threadIdx.x]);
    }
}

__global__ void bn_finalize_kernel(const double* __restrict__ ws, int rows_per_group, int C, int groups, float* __restrict__ mean,
                                   float* __restrict__ rstd, float* __restrict__ rmean, float* __restrict__ rvar,
                                   int64_t* __restrict__ nbt, float eps, float momentum, int repeats) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        float rm = rmean ? rmean[c] : 0.f, rv = rvar ? rvar[c] : 0.f;
        for (int g = 0; g < groups; ++g) {
            const BnMoments st = bn_moments(ws[((long)g * 2 + 0) * C + c], ws[((long)g * 2 + 1) * C + c], (double)rows_per_group, eps);
            mean[g * C + c] = st.mf;
            rstd[g * C + c] = st.rs;
            bn_running(rm, rv, st, momentum, repeats);
        }
        if (rmean) rmean[c] = rm;
        if (rvar) rvar[c] = rv;
    }
    if (c == 0 && nbt) *nbt += (int64_t)groups * repeats;
}

__global__ void bn_eval_stats_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar, int C, float eps,
                                     float* __restrict__ mean, float* __restrict__ rstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        mean[c] = rmean[c];
        rstd[c] = 1.f / sqrtf(rvar[c] + eps);
    }
}

// y = act((x - mean) * rstd * gamma + beta); four channels per thread (C % 4 == 0 is all this path asks, so the channel is recomputed per
// element), scalar otherwise
template <bool VEC>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long rows, int C,
                                                       int rows_per_group, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float slope) {
    const int W = VEC ? 4 : 1;
    const long total = rows * C / W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long e = i * W;
        const long row = e / C;
        const int c = (int)(e - row * C);
        const int g = (int)(row / rows_per_group);
        if (VEC) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + e);
            f32x4 o;
#pragma unroll
            for (int q = 0; q < 4; ++q) o[q] = bn_fwd_element(xv[q], mean[g * C + c + q], rstd[g * C + c + q], gamma[c + q], beta[c + q], slope);
            *reinterpret_cast<f32x4*>(y + e) = o;
        } else {
            y[e] = bn_fwd_element(x[e], mean[g * C + c], rstd[g * C + c], gamma[c], beta[c], slope);
        }
    }
}

// ws: [2][C] doubles = (sum dz, sum dz * xhat) of bn_reduce_kernel<true>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx,
                                                           long rows, int C, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float slope,
                                                           const double* __restrict__ ws, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
    if (blockIdx.x == 0 && (int)threadIdx.x < C) bn_param_grads(dgamma, dbeta, threadIdx.x, ws[threadIdx.x], ws[C + threadIdx.x]);
    const long total = rows * C;
    const double inv_n = 1.0 / (double)rows;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c = (int)(e % C);
        const float rs = rstd[c], ga = gamma[c];
        float xh, dz;
        bn_bwd_element(x[e], dy[e], mean[c], rs, ga, beta[c], slope, xh, dz);
        dx[e] = bn_dx_element(xh, dz, ga, rs, ws[c] * inv_n, ws[C + c] * inv_n);
    }
}

// 16-byte version (same conditions as bn_reduce_vec_kernel)
__global__ __launch_bounds__(256) void bn_bwd_apply_vec_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx,
                                                               long rows, int C, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float slope,
                                                               const double* __restrict__ ws, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
    if (blockIdx.x == 0 && (int)threadIdx.x < C) bn_param_grads(dgamma, dbeta, threadIdx.x, ws[threadIdx.x], ws[C + threadIdx.x]);
    const long total4 = rows * C / 4;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    const int c0 = (int)((i0 * 4) % C);
    bn_dx_loop<2>(reinterpret_cast<const f32x4*>(x), reinterpret_cast<const f32x4*>(dy), reinterpret_cast<f32x4*>(dx),
                  bn_channels(mean, rstd, gamma, beta, c0), bn_dx_means(ws, ws + C, c0, 1.0 / (double)rows), slope, i0, step, total4);
}

// ---- small tensors (the discriminator's and the autoencoder's BatchNorms: a few thousand rows): ONE workgroup does statistics,
// running-stat update and normalisation in one launch -- the multi-kernel path costs four launches of ~5 us for microseconds of work.
// 16-byte accesses throughout: with C a multiple of 4 that divides 4096, thread t always sees the same four channels (its element
// index advances by 4096 per iteration).  LDS fp64 atomics of the fold: 1024 / (C / 4) adders per channel, once per pass.
constexpr int BN_SMALL_THREADS = 1024;
constexpr long BN_SMALL_MAX = 1L << 19;          // elements (2 MB): stays in L2 between the two passes

__global__ __launch_bounds__(BN_SMALL_THREADS) void bn_small_train_kernel(
    const float* __restrict__ x, float* __restrict__ y, int rows_per_group, int C, int groups, float* __restrict__ mean, float* __restrict__ rstd,
    float* __restrict__ rmean, float* __restrict__ rvar, int64_t* __restrict__ nbt, const float* __restrict__ gamma,
    const float* __restrict__ beta, float slope, float eps, float momentum, int repeats) {
    __shared__ double sh_a[256], sh_b[256];
    __shared__ float s_mean[256], s_rstd[256];
    const int c0 = (threadIdx.x * 4) % C;
    float rm = 0.f, rv = 0.f;
    if ((int)threadIdx.x < C) { rm = rmean ? rmean[threadIdx.x] : 0.f; rv = rvar ? rvar[threadIdx.x] : 0.f; }
    const long total4 = (long)rows_per_group * C / 4;
    for (int g = 0; g < groups; ++g) {
        const f32x4* xg = reinterpret_cast<const f32x4*>(x) + g * total4;
        bn_lds_zero(sh_a, sh_b, C);
        double s[4], ss[4];
        bn_accumulate<false>(xg, nullptr, BnCh{}, 1.f, threadIdx.x, BN_SMALL_THREADS, total4, s, ss);
        bn_lds_fold(s, ss, sh_a, sh_b, c0);
        __syncthreads();
        if ((int)threadIdx.x < C) {
            const int c = threadIdx.x;
            const BnMoments st = bn_moments(sh_a[c], sh_b[c], (double)rows_per_group, eps);
            mean[g * C + c] = st.mf; rstd[g * C + c] = st.rs;
            s_mean[c] = st.mf; s_rstd[c] = st.rs;
            bn_running(rm, rv, st, momentum, repeats);
        }
        __syncthreads();
        if (y) bn_y_loop<4>(xg, reinterpret_cast<f32x4*>(y) + g * total4, bn_channels(s_mean, s_rstd, gamma, beta, c0), slope, threadIdx.x, BN_SMALL_THREADS, total4);
        __syncthreads();
    }
    if ((int)threadIdx.x < C) {
        if (rmean) rmean[threadIdx.x] = rm;
        if (rvar) rvar[threadIdx.x] = rv;
    }
    if (threadIdx.x == 0 && nbt) *nbt += (int64_t)groups * repeats;
}

__global__ __launch_bounds__(BN_SMALL_THREADS) void bn_small_bwd_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int rows, int C, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
    float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double sh_a[256], sh_b[256];
    const int c0 = (threadIdx.x * 4) % C;
    bn_lds_zero(sh_a, sh_b, C);
    const BnCh ch = bn_channels(mean, rstd, gamma, beta, c0);
    const long total4 = (long)rows * C / 4;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
    const f32x4* dy4 = reinterpret_cast<const f32x4*>(dy);
    double s[4], sx[4];
    bn_accumulate<true>(x4, dy4, ch, slope, threadIdx.x, BN_SMALL_THREADS, total4, s, sx);
    bn_lds_fold(s, sx, sh_a, sh_b, c0);
    __syncthreads();
    if ((int)threadIdx.x < C) bn_param_grads(dgamma, dbeta, threadIdx.x, sh_a[threadIdx.x], sh_b[threadIdx.x]);
    bn_dx_loop<4>(x4, dy4, reinterpret_cast<f32x4*>(dx), ch, bn_dx_means(sh_a, sh_b, c0, 1.0 / (double)rows), slope, threadIdx.x, BN_SMALL_THREADS, total4);
}

// ---- two-launch BatchNorm (train forward: partial sums | finalize + apply; backward: partial sums | finalize + apply) --------------------
// For everything between the single-workgroup kernels above (<= 32 K elements) and -- replacing them -- the zero / stats / finalize / apply
// chain: no zero fill, no atomics (per-workgroup partials combined in fixed order by every workgroup of the second launch), all statistics
// groups of a stacked forward in ONE launch (grid.y), and the backward of several groups likewise (the discriminator step ran one
// single-workgroup launch of 13-16 us per group and layer).
// part layout: [groups][P][2][C] doubles.
__global__ __launch_bounds__(256) void bn2_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy, long rows_per_group, int C,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                          double* __restrict__ part, int det) {
    // dy == nullptr: (sum x, sum x^2); else (sum dz, sum dz xhat) with dz = dy act'(z), statistics of group blockIdx.y at mean/rstd + g C
    // det (tg_set_deterministic): the threads' sums meet in LDS in thread order instead of through fp64 LDS atomics
    __shared__ double sh[2][256];
    __shared__ double sh_det[256][8];
    const int g = blockIdx.y, P = gridDim.x;
    const long total4 = rows_per_group * C / 4;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)P * 256;
    const int c0 = (int)((i0 * 4) % C);
    bn_lds_zero(sh[0], sh[1], C);
    const f32x4* x4 = reinterpret_cast<const f32x4*>(x) + g * total4;
    double s[4], ss[4];
    if (dy == nullptr)
        bn_accumulate<false>(x4, nullptr, BnCh{}, slope, i0, step, total4, s, ss);
    else
        bn_accumulate<true>(x4, reinterpret_cast<const f32x4*>(dy) + g * total4, bn_channels(mean + g * C, rstd + g * C, gamma, beta, c0), slope, i0, step,
                            total4, s, ss);
    if (det) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { sh_det[threadIdx.x][q] = s[q]; sh_det[threadIdx.x][4 + q] = ss[q]; }
        __syncthreads();
        if ((int)threadIdx.x < C) {                    // channel c lives in the threads t == (c >> 2) mod (C / 4), slot c & 3 (step % C == 0: fixed per thread)
            const int c = threadIdx.x;
            double a = 0.0, b = 0.0;
            for (int t = c >> 2; t < 256; t += C / 4) { a += sh_det[t][c & 3]; b += sh_det[t][4 + (c & 3)]; }
            sh[0][c] = a; sh[1][c] = b;
        }
    } else {
        bn_lds_fold(s, ss, sh[0], sh[1], c0);
    }
    __syncthreads();
    if ((int)threadIdx.x < C) {
        double* o = part + (((long)g * P + blockIdx.x) * 2) * C;
        o[threadIdx.x] = sh[0][threadIdx.x];
        o[C + threadIdx.x] = sh[1][threadIdx.x];
    }
}

// totals of group g's P partials into tot[2][C] (LDS), fixed order: thread (c, slice) sums every (256 / C)-th partial, then the slices
__device__ __forceinline__ void bn2_totals(const double* __restrict__ part, int g, int P, int C, double (*tot)[256], double (*sl)[256]) {
    const int S = 256 / C;                       // slices
    const int c = threadIdx.x % C, sidx = threadIdx.x / C;
    double a = 0.0, b = 0.0;
    if (sidx < S) {
#pragma unroll 8
        for (int p = sidx; p < P; p += S) {          // independent loads, eight in flight
            const double* o = part + (((long)g * P + p) * 2) * C;
            a += o[c];
            b += o[C + c];
        }
    }
    sl[0][threadIdx.x] = a;
    sl[1][threadIdx.x] = b;
    __syncthreads();
    if ((int)threadIdx.x < C) {
        double ta = 0.0, tb = 0.0;
        for (int q = 0; q < S; ++q) { ta += sl[0][q * C + c]; tb += sl[1][q * C + c]; }
        tot[0][c] = ta;
        tot[1][c] = tb;
    }
    __syncthreads();
}

// many partials (large tensors): combined once per group by this launch instead of by every workgroup of the apply launch
__global__ __launch_bounds__(256) void bn2_reduce_kernel(const double* __restrict__ part, int P, int C, double* __restrict__ out) {
    __shared__ double tot[2][256], sl[2][256];
    bn2_totals(part, blockIdx.x, P, C, tot, sl);
    if ((int)threadIdx.x < C) {
        out[((long)blockIdx.x * 2) * C + threadIdx.x] = tot[0][threadIdx.x];
        out[((long)blockIdx.x * 2 + 1) * C + threadIdx.x] = tot[1][threadIdx.x];
    }
}

__global__ __launch_bounds__(256) void bn2_fwd_apply_kernel(const float* __restrict__ x, float* __restrict__ y, long rows_per_group, int C, int groups,
                                                            const double* __restrict__ part, int P, float* __restrict__ mean, float* __restrict__ rstd,
                                                            float* __restrict__ rmean, float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float slope, float eps,
                                                            float momentum, int repeats) {
    __shared__ double tot[2][256], sl[2][256];
    __shared__ float s_mean[256], s_rstd[256];
    const int g = blockIdx.y;
    const double n = (double)rows_per_group;
    if (blockIdx.x == 0 && g == 0) {
        // running statistics: the groups are successive forward calls of the same module -- updated in call order by one workgroup
        float rm = 0.f, rv = 0.f;
        if ((int)threadIdx.x < C) { rm = rmean ? rmean[threadIdx.x] : 0.f; rv = rvar ? rvar[threadIdx.x] : 0.f; }
        for (int gg = 0; gg < groups; ++gg) {
            bn2_totals(part, gg, P, C, tot, sl);
            if ((int)threadIdx.x < C) bn_running(rm, rv, bn_moments(tot[0][threadIdx.x], tot[1][threadIdx.x], n, eps), momentum, repeats);
            __syncthreads();
        }
        if ((int)threadIdx.x < C) {
            if (rmean) rmean[threadIdx.x] = rm;
            if (rvar) rvar[threadIdx.x] = rv;
        }
        if (threadIdx.x == 0 && nbt) *nbt += (int64_t)groups * repeats;
    }
    bn2_totals(part, g, P, C, tot, sl);
    if ((int)threadIdx.x < C) {
        const int c = threadIdx.x;
        const BnMoments st = bn_moments(tot[0][c], tot[1][c], n, eps);
        s_mean[c] = st.mf; s_rstd[c] = st.rs;
        if (blockIdx.x == 0) { mean[g * C + c] = st.mf; rstd[g * C + c] = st.rs; }
    }
    __syncthreads();
    if (y == nullptr) return;
    const long total4 = rows_per_group * C / 4;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    const int c0 = (int)((i0 * 4) % C);
    bn_y_loop<4>(reinterpret_cast<const f32x4*>(x) + g * total4, reinterpret_cast<f32x4*>(y) + g * total4, bn_channels(s_mean, s_rstd, gamma, beta, c0), slope,
                 i0, step, total4);
}

__global__ __launch_bounds__(256) void bn2_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx,
                                                            long rows_per_group, int C, int groups, const double* __restrict__ part, int P,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float slope,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double tot[2][256], sl[2][256];
    const int g = blockIdx.y;
    if (blockIdx.x == 0 && g == 0 && (dgamma || dbeta)) {
        double a = 0.0, b = 0.0;                 // parameter gradients: the groups' sums in group order, one workgroup
        for (int gg = 0; gg < groups; ++gg) {
            bn2_totals(part, gg, P, C, tot, sl);
            if ((int)threadIdx.x < C) { a += tot[0][threadIdx.x]; b += tot[1][threadIdx.x]; }
            __syncthreads();
        }
        if ((int)threadIdx.x < C) bn_param_grads(dgamma, dbeta, threadIdx.x, a, b);
    }
    bn2_totals(part, g, P, C, tot, sl);
    const long total4 = rows_per_group * C / 4;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    const int c0 = (int)((i0 * 4) % C);
    bn_dx_loop<2>(reinterpret_cast<const f32x4*>(x) + g * total4, reinterpret_cast<const f32x4*>(dy) + g * total4, reinterpret_cast<f32x4*>(dx) + g * total4,
                  bn_channels(mean + g * C, rstd + g * C, gamma, beta, c0), bn_dx_means(tot[0], tot[1], c0, 1.0 / (double)rows_per_group), slope, i0, step,
                  total4);
}

// 16-byte kernels: a thread keeps the same four channels across its grid-stride loop
inline bool bn_vec_ok(int C, long elems) { return C >= 4 && C <= 256 && C % 4 == 0 && 1024 % C == 0 && elems % 4 == 0; }
// grids of the streaming reduce kernels: eight 16-byte elements per thread; sixteen rows per thread of the scalar form, at most 1024 workgroups
inline int bn_vec_grid(long total4) { return ew_grid(total4, 256, 8); }
inline int bn_scalar_grid(int rows, int C) {
    const int blocks = cdiv(rows, (256 / C) * 16);
    return blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
}

}  // namespace tg

using namespace tg;

extern "C" int32_t tg_bn_fused_supported(int32_t rows, int32_t C, int32_t groups) {
    return C >= 4 && C <= 256 && C % 4 == 0 && 4096 % C == 0 && groups > 0 && rows > 0 && rows % groups == 0 && (long)rows * C <= BN_SMALL_MAX &&
           ((long)(rows / groups) * C) % 4 == 0;
}

// statistics + running-stat update + normalisation of a small tensor in ONE launch (y may be NULL: statistics only)
extern "C" int tg_bn_train_fused(const float* x, float* y, int32_t rows, int32_t C, int32_t groups, float* mean, float* rstd,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                                 const float* beta, float act_slope, float eps, float momentum, int32_t repeats, void* stream) {
    TG_REQUIRE(x && mean && rstd && repeats >= 1 && (y == nullptr || (gamma && beta)), "tg_bn_train_fused: null pointer / repeats < 1");
    TG_REQUIRE(tg_bn_fused_supported(rows, C, groups) && aligned16(x) && (y == nullptr || aligned16(y)),
               "tg_bn_train_fused: unsupported shape C=%d rows=%d groups=%d (see tg_bn_fused_supported) or unaligned pointers", C, rows, groups);
    hipLaunchKernelGGL(bn_small_train_kernel, dim3(1), dim3(BN_SMALL_THREADS), 0, (hipStream_t)stream, x, y, rows / groups, C, groups, mean, rstd,
                       running_mean, running_var, num_batches_tracked, gamma, beta, act_slope, eps, momentum, repeats);
    return check_launch("tg_bn_train_fused");
}

extern "C" int tg_bn_train_stats(const float* x, int32_t rows, int32_t C, int32_t groups, double* ws, float* mean, float* rstd,
                                 float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                                 float momentum, int32_t repeats, void* stream) {
    TG_REQUIRE(x && ws && mean && rstd && repeats >= 1, "tg_bn_train_stats: null pointer / repeats < 1");
    TG_REQUIRE(C > 0 && C <= 256 && groups > 0 && rows > 0 && rows % groups == 0, "tg_bn_train_stats: C=%d (<=256), rows=%d, groups=%d", C, rows, groups);
    hipStream_t s = (hipStream_t)stream;
    if (zero_async(ws, sizeof(double) * 2 * (size_t)groups * C, s)) return 1;
    const int rpg = rows / groups;
    const float* none = nullptr;
    if (bn_vec_ok(C, (long)rpg * C) && aligned16(x))
        hipLaunchKernelGGL(bn_reduce_vec_kernel<false>, dim3(bn_vec_grid((long)rpg * C / 4), groups), dim3(256), 0, s, x, none, (long)rpg, C, none, none, none, none, 1.f, ws);
    else
        hipLaunchKernelGGL(bn_reduce_kernel<false>, dim3(bn_scalar_grid(rpg, C), groups), dim3(256), 0, s, x, none, rpg, C, none, none, none, none, 1.f, ws);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, ws, rpg, C, groups, mean, rstd, running_mean, running_var,
                       num_batches_tracked, eps, momentum, repeats);
    return check_launch("tg_bn_train_stats");
}

extern "C" int tg_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps, float* mean,
                                float* rstd, void* stream) {
    TG_REQUIRE(running_mean && running_var && mean && rstd && C > 0, "tg_bn_eval_stats: bad arguments");
    hipLaunchKernelGGL(bn_eval_stats_kernel, dim3(cdiv(C, 64)), dim3(64), 0, (hipStream_t)stream, running_mean, running_var, C, eps, mean, rstd);
    return check_launch("tg_bn_eval_stats");
}

extern "C" int tg_bn_apply(const float* x, float* y, int32_t rows, int32_t C, int32_t groups, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, float act_slope, void* stream) {
    TG_REQUIRE(x && y && mean && rstd && gamma && beta, "tg_bn_apply: null pointer");
    TG_REQUIRE(rows > 0 && C > 0 && groups > 0 && rows % groups == 0, "tg_bn_apply: bad sizes");
    const bool vec = (C % 4 == 0) && aligned16(x) && aligned16(y);
    const long total = (long)rows * C;
    if (vec) hipLaunchKernelGGL((bn_apply_kernel<true>), dim3(ew_grid(total / 4, 256, 2)), dim3(256), 0, (hipStream_t)stream, x, y, (long)rows, C, rows / groups, mean, rstd, gamma, beta, act_slope);
    else     hipLaunchKernelGGL((bn_apply_kernel<false>), dim3(ew_grid(total, 256, 4)), dim3(256), 0, (hipStream_t)stream, x, y, (long)rows, C, rows / groups, mean, rstd, gamma, beta, act_slope);
    return check_launch("tg_bn_apply");
}

extern "C" int tg_bn_backward(const float* dy, const float* x, float* dx, int32_t rows, int32_t C, const float* mean,
                              const float* rstd, const float* gamma, const float* beta, float act_slope, double* ws,
                              float* dgamma, float* dbeta, void* stream) {
    TG_REQUIRE(dy && x && dx && mean && rstd && gamma && beta && ws, "tg_bn_backward: null pointer");
    TG_REQUIRE(rows > 0 && C > 0 && C <= 256, "tg_bn_backward: C=%d must be <= 256", C);
    hipStream_t s = (hipStream_t)stream;
    if (tg_bn_fused_supported(rows, C, 1) && aligned16(dy) && aligned16(x) && aligned16(dx)) {   // one workgroup: reduce, then apply (3 launches -> 1)
        hipLaunchKernelGGL(bn_small_bwd_kernel, dim3(1), dim3(BN_SMALL_THREADS), 0, s, dy, x, dx, rows, C, mean, rstd, gamma, beta, act_slope,
                           dgamma, dbeta);
        return check_launch("tg_bn_backward(small)");
    }
    if (zero_async(ws, sizeof(double) * 2 * (size_t)C, s)) return 1;
    if (bn_vec_ok(C, (long)rows * C) && aligned16(dy) && aligned16(x) && aligned16(dx)) {
        const int vb = bn_vec_grid((long)rows * C / 4);
        hipLaunchKernelGGL(bn_reduce_vec_kernel<true>, dim3(vb), dim3(256), 0, s, x, dy, (long)rows, C, mean, rstd, gamma, beta, act_slope, ws);
        hipLaunchKernelGGL(bn_bwd_apply_vec_kernel, dim3(vb), dim3(256), 0, s, dy, x, dx, (long)rows, C, mean, rstd, gamma, beta, act_slope, ws,
                           dgamma, dbeta);
        return check_launch("tg_bn_backward(vec)");
    }
    hipLaunchKernelGGL(bn_reduce_kernel<true>, dim3(bn_scalar_grid(rows, C)), dim3(256), 0, s, x, dy, rows, C, mean, rstd, gamma, beta, act_slope, ws);
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_grid((long)rows * C, 256, 4)), dim3(256), 0, s, dy, x, dx, (long)rows, C, mean, rstd,
                       gamma, beta, act_slope, ws, dgamma, dbeta);
    return check_launch("tg_bn_backward");
}

// ---- two-launch forms (csrc/norm.hip bn2_*): all `groups` statistics groups of x [groups * rows_per_group][C] in one pair of launches.
extern "C" int32_t tg_bn2_supported(int32_t rows_per_group, int32_t C) {
    return rows_per_group > 0 && bn_vec_ok(C, (long)rows_per_group * C) && 256 % C == 0;
}
static int bn2_parts(long rows_per_group, int C) {
    long p = (rows_per_group * C / 4 + 2047) / 2048;
    return (int)(p < 1 ? 1 : (p > 256 ? 256 : p));
}
constexpr int BN2_INLINE_PARTS = 32;          // up to this many partials every apply workgroup combines them itself; beyond, one reduce launch
extern "C" int64_t tg_bn2_ws_doubles(int32_t rows_per_group, int32_t C, int32_t groups) {
    return tg_bn2_supported(rows_per_group, C) && groups > 0 ? (int64_t)groups * (bn2_parts(rows_per_group, C) + 1) * 2 * C : 0;
}
// partial sums of all groups -> (pointer, count) the apply launch reads
static const double* bn2_combine(double* ws, int P, int C, int groups, int* p_out, hipStream_t s) {
    if (P <= BN2_INLINE_PARTS) { *p_out = P; return ws; }
    double* tot = ws + (long)groups * P * 2 * C;
    hipLaunchKernelGGL(bn2_reduce_kernel, dim3(groups), dim3(256), 0, s, ws, P, C, tot);
    *p_out = 1;
    return tot;
}

extern "C" int tg_bn2_train(const float* x, float* y, int32_t rows_per_group, int32_t C, int32_t groups, double* ws, int64_t ws_doubles, float* mean,
                            float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                            const float* beta, float act_slope, float eps, float momentum, int32_t repeats, void* stream) {
    TG_REQUIRE(x && ws && mean && rstd && groups > 0 && repeats >= 1 && (y == nullptr || (gamma && beta)), "tg_bn2_train: null pointer / bad counts");
    TG_REQUIRE(tg_bn2_supported(rows_per_group, C) && aligned16(x) && (y == nullptr || aligned16(y)), "tg_bn2_train: unsupported shape C=%d rows=%d (tg_bn2_supported) or unaligned pointers", C, rows_per_group);
    TG_REQUIRE(ws_doubles >= tg_bn2_ws_doubles(rows_per_group, C, groups), "tg_bn2_train: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int P = bn2_parts(rows_per_group, C);
    hipLaunchKernelGGL(bn2_partial_kernel, dim3(P, groups), dim3(256), 0, s, x, (const float*)nullptr, (long)rows_per_group, C, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 1.f, ws, deterministic() ? 1 : 0);
    int Pa;
    const double* tot = bn2_combine(ws, P, C, groups, &Pa, s);
    hipLaunchKernelGGL(bn2_fwd_apply_kernel, dim3(P, groups), dim3(256), 0, s, x, y, (long)rows_per_group, C, groups, tot, Pa, mean, rstd, running_mean,
                       running_var, num_batches_tracked, gamma, beta, act_slope, eps, momentum, repeats);
    return check_launch("tg_bn2_train");
}

extern "C" int tg_bn2_backward(const float* dy, const float* x, float* dx, int32_t rows_per_group, int32_t C, int32_t groups, const float* mean,
                               const float* rstd, const float* gamma, const float* beta, float act_slope, double* ws, int64_t ws_doubles,
                               float* dgamma, float* dbeta, void* stream) {
    TG_REQUIRE(dy && x && dx && mean && rstd && gamma && beta && ws && groups > 0, "tg_bn2_backward: null pointer / bad counts");
    TG_REQUIRE(tg_bn2_supported(rows_per_group, C) && aligned16(dy) && aligned16(x) && aligned16(dx), "tg_bn2_backward: unsupported shape C=%d rows=%d or unaligned pointers", C, rows_per_group);
    TG_REQUIRE(ws_doubles >= tg_bn2_ws_doubles(rows_per_group, C, groups), "tg_bn2_backward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int P = bn2_parts(rows_per_group, C);
    hipLaunchKernelGGL(bn2_partial_kernel, dim3(P, groups), dim3(256), 0, s, x, dy, (long)rows_per_group, C, mean, rstd, gamma, beta, act_slope, ws, deterministic() ? 1 : 0);
    int Pa;
    const double* tot = bn2_combine(ws, P, C, groups, &Pa, s);
    hipLaunchKernelGGL(bn2_bwd_apply_kernel, dim3(P, groups), dim3(256), 0, s, dy, x, dx, (long)rows_per_group, C, groups, tot, Pa, mean, rstd, gamma, beta,
                       act_slope, dgamma, dbeta);
    return check_launch("tg_bn2_backward");
}
