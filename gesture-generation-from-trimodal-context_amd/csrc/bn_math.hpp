// The BatchNorm arithmetic of csrc/norm.hip, each formula, sum and 16-byte loop stated once.  The association rules
// below are what tests/test_bn_envelope_gpu.py gates against fp64 and tests/test_bn_parent_bits_gpu.py pins bit for bit.
#pragma once
#include "common.hpp"

namespace tg {

// ---- moments of one statistics group and channel, from its fp64 sums over n rows
struct BnMoments {
    double m, var, unbiased;                     // var: biased, E[x^2] - m^2 clamped at 0 (cancellation can leave it below); unbiased = var for one row
    float mf, rs;                                // (float)m and rstd: what the kernels store and normalise with
};
__device__ __forceinline__ BnMoments bn_moments(double sum, double sumsq, double n, float eps) {
    BnMoments o;
    o.m = sum / n;
    o.var = sumsq / n - o.m * o.m;
    if (o.var < 0.0) o.var = 0.0;
    o.mf = (float)o.m;
    o.rs = (float)(1.0 / sqrt(o.var + (double)eps));
    o.unbiased = n > 1.0 ? o.var * n / (n - 1.0) : o.var;
    return o;
}
// the same batch normalised by `repeats` identical forward calls.  The running mean takes mf == (float)m: one expression for every caller
__device__ __forceinline__ void bn_running(float& rm, float& rv, const BnMoments& s, float momentum, int repeats) {
    for (int q = 0; q < repeats; ++q) {
        rm = (1.f - momentum) * rm + momentum * s.mf;
        rv = (1.f - momentum) * rv + momentum * (float)s.unbiased;
    }
}

// ---- elements
// y = act((x - mean) * rstd * gamma + beta), in this association
__device__ __forceinline__ float bn_fwd_element(float v, float mu, float rs, float ga, float be, float slope) {
    return act_fn((v - mu) * rs * ga + be, slope);
}
// xhat and dz = dy act'(z); the derivative at z == 0 is `slope`
__device__ __forceinline__ void bn_bwd_element(float xv, float dv, float mu, float rs, float ga, float be, float slope, float& xh, float& dz) {
    xh = (xv - mu) * rs;
    const float z = xh * ga + be;
    dz = dv * (z > 0.f ? 1.f : slope);
}
// m1, m2: the batch means of dz and dz xhat.  They are subtracted in fp64: rounding them to fp32 first would shift every element of the
// channel by the same amount, and the next layer's weight-gradient sum over ~1e6 rows amplifies that coherently
__device__ __forceinline__ float bn_dx_element(float xh, float dz, float ga, float rs, double m1, double m2) {
    return (float)((double)(ga * rs) * ((double)dz - m1 - (double)xh * m2));
}
__device__ __forceinline__ void bn_param_grads(float* __restrict__ dgamma, float* __restrict__ dbeta, int c, double sum_dz, double sum_dz_xh) {
    if (dbeta) dbeta[c] += (float)sum_dz;
    if (dgamma) dgamma[c] += (float)sum_dz_xh;
}

// ---- the 16-byte forms.  A thread's element index advances by a multiple of C, so its four channels c0 .. c0 + 3 never change: their
// constants are registers, the partial sums eight fp64 registers, and the loads of successive iterations are independent requests
struct BnCh { float mu[4], rs[4], ga[4], be[4]; };
struct BnDx { double m1[4], m2[4]; };
// mean / rstd: this group's [C], in global memory or LDS
__device__ __forceinline__ BnCh bn_channels(const float* mean, const float* rstd, const float* __restrict__ gamma, const float* __restrict__ beta, int c0) {
    BnCh ch;
#pragma unroll
    for (int q = 0; q < 4; ++q) { ch.mu[q] = mean[c0 + q]; ch.rs[q] = rstd[c0 + q]; ch.ga[q] = gamma[c0 + q]; ch.be[q] = beta[c0 + q]; }
    return ch;
}
__device__ __forceinline__ BnDx bn_dx_means(const double* sum_dz, const double* sum_dz_xh, int c0, double inv_n) {
    BnDx d;
#pragma unroll
    for (int q = 0; q < 4; ++q) { d.m1[q] = sum_dz[c0 + q] * inv_n; d.m2[q] = sum_dz_xh[c0 + q] * inv_n; }
    return d;
}

// forward: (sum x, sum x^2); backward: (sum dz, sum dz xhat), over the elements i0, i0 + step, ... < total4
template <bool BWD>
__device__ __forceinline__ void bn_accumulate(const f32x4* __restrict__ x4, const f32x4* __restrict__ dy4, const BnCh& ch, float slope, long i0, long step,
                                              long total4, double (&s)[4], double (&ss)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] = ss[q] = 0.0;
#pragma unroll 4
    for (long i = i0; i < total4; i += step) {
        const f32x4 xv = x4[i];
        if constexpr (BWD) {
            const f32x4 dv = dy4[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float xh, dz;
                bn_bwd_element(xv[q], dv[q], ch.mu[q], ch.rs[q], ch.ga[q], ch.be[q], slope, xh, dz);
                s[q] += dz;
                ss[q] += (double)dz * xh;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) { s[q] += xv[q]; ss[q] += (double)xv[q] * xv[q]; }
        }
    }
}
template <int UNROLL>
__device__ __forceinline__ void bn_y_loop(const f32x4* __restrict__ x4, f32x4* __restrict__ y4, const BnCh& ch, float slope, long i0, long step, long total4) {
#pragma unroll UNROLL
    for (long i = i0; i < total4; i += step) {
        const f32x4 v = x4[i];
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = bn_fwd_element(v[q], ch.mu[q], ch.rs[q], ch.ga[q], ch.be[q], slope);
        y4[i] = o;
    }
}
template <int UNROLL>
__device__ __forceinline__ void bn_dx_loop(const f32x4* __restrict__ x4, const f32x4* __restrict__ dy4, f32x4* __restrict__ dx4, const BnCh& ch, const BnDx& d,
                                           float slope, long i0, long step, long total4) {
#pragma unroll UNROLL
    for (long i = i0; i < total4; i += step) {
        const f32x4 xv = x4[i], dv = dy4[i];
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float xh, dz;
            bn_bwd_element(xv[q], dv[q], ch.mu[q], ch.rs[q], ch.ga[q], ch.be[q], slope, xh, dz);
            o[q] = bn_dx_element(xh, dz, ch.ga[q], ch.rs[q], d.m1[q], d.m2[q]);
        }
        dx4[i] = o;
    }
}

// ---- per-channel totals of a workgroup in LDS: sh_a / sh_b are [C] accumulators, zeroed (with the barrier), then every thread adds its
// four pairs by fp64 LDS atomics (threads with equal c0 hold the same channels); the caller places the barrier before it reads them
__device__ __forceinline__ void bn_lds_zero(double* sh_a, double* sh_b, int C) {
    if ((int)threadIdx.x < C) { sh_a[threadIdx.x] = 0.0; sh_b[threadIdx.x] = 0.0; }
    __syncthreads();
}
__device__ __forceinline__ void bn_lds_fold(const double (&a)[4], const double (&b)[4], double* sh_a, double* sh_b, int c0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { atomicAdd(&sh_a[c0 + q], a[q]); atomicAdd(&sh_b[c0 + q], b[q]); }
}

}  // namespace tg
