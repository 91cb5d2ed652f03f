// Latent-head MLPs of the joint-embedding baseline (model/embedding_net.py: ContextEncoder.out + fc_mu / fc_logvar + reparameterize :230-259,
// PoseDecoderGRU.pre_pose_net :138-143): Linear(K0, N1) -> BatchNorm1d(N1) over the batch -> activation -> Linear(N1, N2) [-> fc_mu, fc_logvar
// (N2 x N2 each) -> z = mu + eps exp(logvar / 2)], ONE launch each way.
//
// Organisation: ONE workgroup of 512 threads.  The work is a few MFLOP at most and the BatchNorm statistics need every row of the first
// linear before any row of the second, so a grid would need a device-wide hand-off for microseconds of arithmetic; a single workgroup needs
// only its own barriers, cannot hang on co-residency and sums everything in an order fixed by the shape alone (no atomics: two runs are bit
// identical).  All products go through one tiled routine (mm): the weight chunk and the activation chunk of 32 reduction indices are staged
// in LDS, every thread owns one output column and 8 rows, and each output element is ONE fp32 FMA chain over the reduction index in ascending
// order -- independent of the batch size and of the row's position, so in eval mode (BatchNorm on running statistics) row b of a batch
// equals that row run alone bit for bit.  Batch statistics and the BatchNorm backward sums accumulate in fp64 (as csrc/norm.hip).
// Intermediates (the pre-BatchNorm activations h1, which the backward reads again, and scratch) live in global memory: they are written and
// read by this one workgroup with a barrier in between.
#include "common.hpp"

namespace tg {
namespace {

constexpr int LH_THREADS = 512;
constexpr int LH_MAX_B = 512, LH_MAX_K0 = 384, LH_MAX_N1 = 256, LH_MAX_N2 = 64;
constexpr int LH_KC = 32;            // reduction indices per staged chunk
constexpr int LH_R = 8;              // rows per thread
constexpr int LH_XS_LD = 36;         // padded chunk row (16-byte aligned rows)

struct LhShared {
    float w[LH_KC][256 + 1];                               // [reduction index][output column]
    float x[(LH_THREADS / 32) * LH_R][LH_XS_LD] __attribute__((aligned(16)));           // [row][reduction index]
    double red[LH_THREADS];
};

__device__ __forceinline__ int lh_cols(int n) {           // column tile: power of two in [32, 256]
    int c = 32;
    while (c < n && c < 256) c <<= 1;
    return c;
}

// Y[m][n] (+)= bias[n] + sum_j Xop(m, j) Wop(j, n), m < M, n < N, j < J.
// Xop(m, j) = XT ? X[j * ldx + m] : X[m * ldx + j];  Wop(j, n) = WJ ? W[j * ldw + n] : W[n * ldw + j].
template <bool XT, bool WJ>
__device__ void mm(LhShared& S, const float* X, long ldx, const float* W, long ldw, const float* bias, float* Y, long ldy, int M, int N, int J,
                   bool accumulate) {
    const int t = threadIdx.x;
    const int NC = lh_cols(N), G = LH_THREADS / NC, RP = G * LH_R;
    const int c = t % NC, g = t / NC;
    for (int n0 = 0; n0 < N; n0 += NC) {
        for (int m0 = 0; m0 < M; m0 += RP) {
            float acc[LH_R];
#pragma unroll
            for (int r = 0; r < LH_R; ++r) acc[r] = 0.f;
            for (int j0 = 0; j0 < J; j0 += LH_KC) {
                __syncthreads();
                for (int i = t; i < NC * LH_KC; i += LH_THREADS) {
                    int jj, cc;
                    if (WJ) { jj = i / NC; cc = i % NC; } else { cc = i / LH_KC; jj = i % LH_KC; }
                    const int j = j0 + jj, n = n0 + cc;
                    float v = 0.f;
                    if (j < J && n < N) v = WJ ? W[(long)j * ldw + n] : W[(long)n * ldw + j];
                    S.w[jj][cc] = v;
                }
                for (int i = t; i < RP * LH_KC; i += LH_THREADS) {
                    int jj, r;
                    if (XT) { jj = i / RP; r = i % RP; } else { r = i / LH_KC; jj = i % LH_KC; }
                    const int j = j0 + jj, m = m0 + r;
                    float v = 0.f;
                    if (j < J && m < M) v = XT ? X[(long)j * ldx + m] : X[(long)m * ldx + j];
                    S.x[r][jj] = v;
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < LH_KC / 4; ++q) {
                    const float w0 = S.w[4 * q][c], w1 = S.w[4 * q + 1][c], w2 = S.w[4 * q + 2][c], w3 = S.w[4 * q + 3][c];
#pragma unroll
                    for (int r = 0; r < LH_R; ++r) {
                        const f32x4 xv = *reinterpret_cast<const f32x4*>(&S.x[g * LH_R + r][4 * q]);
                        float a = acc[r];
                        a = fmaf(xv[0], w0, a); a = fmaf(xv[1], w1, a); a = fmaf(xv[2], w2, a); a = fmaf(xv[3], w3, a);
                        acc[r] = a;
                    }
                }
            }
            const int n = n0 + c;
            if (n < N) {
                const float bv = bias ? bias[n] : 0.f;
#pragma unroll
                for (int r = 0; r < LH_R; ++r) {
                    const int m = m0 + g * LH_R + r;
                    if (m < M) {
                        float* y = Y + (long)m * ldy + n;
                        const float v = acc[r] + bv;
                        *y = accumulate ? *y + v : v;
                    }
                }
            }
        }
    }
    __syncthreads();
}

// sums over the rows of up to two per-element terms per column, fp64, fixed order: column n = t % NC, part p = t / NC takes rows p, p + P, ..;
// the parts are added in ascending order.  f(b, n, s0, s1) adds its terms.  Results for n < N in out0 / out1 (LDS-free: returned through S.red).
template <typename F>
__device__ void col_sums(LhShared& S, int B, int N, F f, double* out0, double* out1) {
    const int t = threadIdx.x, NC = lh_cols(N), P = LH_THREADS / NC, n = t % NC, p = t / NC;
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && out1 == nullptr) break;
        double s0 = 0.0, s1 = 0.0;
        if (n < N)
            for (int b = p; b < B; b += P) f(b, n, s0, s1);
        __syncthreads();
        S.red[t] = pass == 0 ? s0 : s1;
        __syncthreads();
        if (p == 0 && n < N) {
            double s = 0.0;
            for (int q = 0; q < P; ++q) s += S.red[q * NC + n];
            (pass == 0 ? out0 : out1)[n] = s;
        }
    }
    __syncthreads();
}

struct LhFwd {
    const float* x; long ldx;
    const float *W1, *b1, *gamma, *beta;
    float *rmean, *rvar; int64_t* nbt;
    const float *W2, *b2, *Wmu, *bmu, *Wlv, *blv;
    float* eps; const uint64_t* rng; uint32_t site;
    float* out; long ldo;
    float *h1, *act; double* stats; float *h2, *mu, *logvar;
    int B, K0, N1, N2, training;
    float slope, bn_eps, momentum;
};

__global__ __launch_bounds__(LH_THREADS) void latent_head_fwd_kernel(LhFwd a) {
    __shared__ LhShared S;
    __shared__ double cs0[LH_MAX_N1], cs1[LH_MAX_N1];
    const int t = threadIdx.x, B = a.B, N1 = a.N1, N2 = a.N2;
    mm<false, false>(S, a.x, a.ldx, a.W1, a.K0, a.b1, a.h1, N1, B, N1, a.K0, false);
    double* mean = a.stats;                 // fp64: with few rows the BatchNorm backward cancels almost completely (B = 2: a factor 1 - xhat^2 ~ eps)
    double* rstd = a.stats + N1;
    if (a.training) {
        const float* h1 = a.h1;
        col_sums(S, B, N1, [&](int b, int n, double& s0, double&) { s0 += (double)h1[(long)b * N1 + n]; }, cs0, nullptr);
        if (t < N1) cs0[t] = cs0[t] / B;
        __syncthreads();
        col_sums(S, B, N1, [&](int b, int n, double& s0, double&) { const double d = (double)h1[(long)b * N1 + n] - cs0[n]; s0 += d * d; }, cs1, nullptr);
        if (t < N1) {
            const double m = cs0[t], var = cs1[t] / B, unb = cs1[t] / (B - 1);
            mean[t] = m;
            rstd[t] = 1.0 / sqrt(var + (double)a.bn_eps);
            a.rmean[t] = (1.f - a.momentum) * a.rmean[t] + a.momentum * (float)m;
            a.rvar[t] = (1.f - a.momentum) * a.rvar[t] + a.momentum * (float)unb;
        }
        if (t == 0 && a.nbt) *a.nbt += 1;
    } else if (t < N1) {
        mean[t] = (double)a.rmean[t];
        rstd[t] = 1.0 / sqrt((double)a.rvar[t] + (double)a.bn_eps);
    }
    __syncthreads();
    for (int i = t; i < B * N1; i += LH_THREADS) {
        const int n = i % N1;
        const float v = (float)(((double)a.h1[i] - mean[n]) * rstd[n] * (double)a.gamma[n] + (double)a.beta[n]);
        a.act[i] = act_fn(v, a.slope);
    }
    __syncthreads();
    if (!a.Wmu) {
        mm<false, false>(S, a.act, N1, a.W2, N1, a.b2, a.out, a.ldo, B, N2, N1, false);
        return;
    }
    mm<false, false>(S, a.act, N1, a.W2, N1, a.b2, a.h2, N2, B, N2, N1, false);
    mm<false, false>(S, a.h2, N2, a.Wmu, N2, a.bmu, a.mu, N2, B, N2, N2, false);
    mm<false, false>(S, a.h2, N2, a.Wlv, N2, a.blv, a.logvar, N2, B, N2, N2, false);
    for (int i = t; i < B * N2; i += LH_THREADS) {
        float e;
        if (a.rng) {                                         // element i of tg_normal(eps, B * N2, state, site), bit for bit (as csrc/speaker.hip)
            uint32_t r[4];
            philox4x32(a.rng[0], (uint64_t)(i >> 2), a.site, (uint32_t)a.rng[1], r);
            const int q = (i & 3) >> 1;
            const float rad = sqrtf(-2.f * logf(u01(r[2 * q])));
            const float ang = 6.283185307179586f * u01(r[2 * q + 1]);
            e = (i & 1) ? rad * sinf(ang) : rad * cosf(ang);
            a.eps[i] = e;
        } else {
            e = a.eps[i];
        }
        a.out[(long)(i / N2) * a.ldo + i % N2] = a.mu[i] + e * expf(0.5f * a.logvar[i]);
    }
}

struct LhBwd {
    const float* dout; long ldo;
    const float *dmu, *dlv;
    const float* x; long ldx;
    const float *W1, *gamma, *beta, *W2, *Wmu, *Wlv, *eps, *h1; const double* stats; const float *h2, *logvar;
    float* ws;
    float *dW1, *db1, *dgamma, *dbeta, *dW2, *db2, *dWmu, *dbmu, *dWlv, *dblv;
    float* dx; long lddx;
    int B, K0, N1, N2, training;
    float slope;
};

template <typename F>
__device__ void col_sum_to(LhShared& S, double* tmp, int B, int N, F f, float* out) {
    col_sums(S, B, N, f, tmp, nullptr);
    if ((int)threadIdx.x < N) out[threadIdx.x] = (float)tmp[threadIdx.x];
    __syncthreads();
}

__global__ __launch_bounds__(LH_THREADS) void latent_head_bwd_kernel(LhBwd a) {
    __shared__ LhShared S;
    __shared__ double cs0[LH_MAX_N1], cs1[LH_MAX_N1];
    const int t = threadIdx.x, B = a.B, N1 = a.N1, N2 = a.N2, K0 = a.K0;
    float* act = a.ws;                       // [B][N1]
    float* da = act + (long)B * N1;          // [B][N1]: d act, then d h1 in place
    float* dm = da + (long)B * N1;           // [B][N2] (tail)
    float* dl = dm + (long)B * N2;           // [B][N2] (tail)
    float* dh2w = dl + (long)B * N2;         // [B][N2] (tail)
    const double* mean = a.stats;
    const double* rstd = a.stats + N1;
    const float* dh2 = a.dout;
    long ldh2 = a.ldo;
    if (a.Wmu) {
        for (int i = t; i < B * N2; i += LH_THREADS) {
            const float dz = a.dout[(long)(i / N2) * a.ldo + i % N2];
            dm[i] = dz + (a.dmu ? a.dmu[i] : 0.f);
            dl[i] = dz * a.eps[i] * 0.5f * expf(0.5f * a.logvar[i]) + (a.dlv ? a.dlv[i] : 0.f);
        }
        __syncthreads();
        mm<true, true>(S, dm, N2, a.h2, N2, nullptr, a.dWmu, N2, N2, N2, B, false);
        mm<true, true>(S, dl, N2, a.h2, N2, nullptr, a.dWlv, N2, N2, N2, B, false);
        col_sum_to(S, cs0, B, N2, [&](int b, int n, double& s0, double&) { s0 += (double)dm[(long)b * N2 + n]; }, a.dbmu);
        col_sum_to(S, cs0, B, N2, [&](int b, int n, double& s0, double&) { s0 += (double)dl[(long)b * N2 + n]; }, a.dblv);
        mm<false, true>(S, dm, N2, a.Wmu, N2, nullptr, dh2w, N2, B, N2, N2, false);
        mm<false, true>(S, dl, N2, a.Wlv, N2, nullptr, dh2w, N2, B, N2, N2, true);
        dh2 = dh2w;
        ldh2 = N2;
    }
    // the activations the forward did not keep
    for (int i = t; i < B * N1; i += LH_THREADS) {
        const int n = i % N1;
        act[i] = act_fn((float)(((double)a.h1[i] - mean[n]) * rstd[n] * (double)a.gamma[n] + (double)a.beta[n]), a.slope);
    }
    __syncthreads();
    mm<true, true>(S, dh2, ldh2, act, N1, nullptr, a.dW2, N1, N2, N1, B, false);
    col_sum_to(S, cs0, B, N2, [&](int b, int n, double& s0, double&) { s0 += (double)dh2[(long)b * ldh2 + n]; }, a.db2);
    mm<false, true>(S, dh2, ldh2, a.W2, N1, nullptr, da, N1, B, N1, N2, false);
    // activation and BatchNorm backward: d pre = d act * act'(pre); dbeta = sum d pre, dgamma = sum d pre * xhat
    for (int i = t; i < B * N1; i += LH_THREADS) {
        const int n = i % N1;
        const float pre = (float)(((double)a.h1[i] - mean[n]) * rstd[n] * (double)a.gamma[n] + (double)a.beta[n]);
        da[i] = pre > 0.f ? da[i] : da[i] * a.slope;
    }
    __syncthreads();
    {
        const float* h1 = a.h1;
        col_sums(S, B, N1, [&](int b, int n, double& s0, double& s1) {
            const double d = (double)da[(long)b * N1 + n];
            s0 += d;
            s1 += d * (((double)h1[(long)b * N1 + n] - mean[n]) * rstd[n]);
        }, cs0, cs1);
    }
    if (t < N1) { a.dbeta[t] = (float)cs0[t]; a.dgamma[t] = (float)cs1[t]; }
    for (int i = t; i < B * N1; i += LH_THREADS) {
        const int n = i % N1;
        const double gr = (double)a.gamma[n] * rstd[n];
        if (a.training) {
            const double xh = ((double)a.h1[i] - mean[n]) * rstd[n];
            da[i] = (float)(gr * ((double)da[i] - (cs0[n] + xh * cs1[n]) / B));
        } else {
            da[i] = (float)(gr * (double)da[i]);
        }
    }
    __syncthreads();
    mm<true, true>(S, da, N1, a.x, a.ldx, nullptr, a.dW1, K0, N1, K0, B, false);
    col_sum_to(S, cs0, B, N1, [&](int b, int n, double& s0, double&) { s0 += (double)da[(long)b * N1 + n]; }, a.db1);
    if (a.dx) mm<false, true>(S, da, N1, a.W1, K0, nullptr, a.dx, a.lddx, B, K0, N1, false);
}

bool lh_shape_ok(int B, int K0, int N1, int N2, int training) {
    return B >= (training ? 2 : 1) && B <= LH_MAX_B && K0 >= 1 && K0 <= LH_MAX_K0 && N1 >= 1 && N1 <= LH_MAX_N1 && N2 >= 1 && N2 <= LH_MAX_N2;
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int tg_latent_head_supported(int32_t B, int32_t K0, int32_t N1, int32_t N2, int32_t training, int32_t* out) {
    TG_REQUIRE(out, "tg_latent_head_supported: null result pointer");
    TG_REQUIRE(B >= 0 && K0 >= 0 && N1 >= 0 && N2 >= 0, "tg_latent_head_supported: negative size");
    *out = lh_shape_ok(B, K0, N1, N2, training) ? 1 : 0;
    return 0;
}

extern "C" int tg_latent_head_fwd(const float* x, int64_t ldx, const float* W1, const float* b1, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, int64_t* nbt, const float* W2, const float* b2, const float* Wmu,
                                  const float* bmu, const float* Wlv, const float* blv, float* eps, const uint64_t* rng_state, uint32_t site,
                                  float* out, int64_t ldo, float* h1, float* act_ws, double* stats, float* h2, float* mu, float* logvar, int32_t B,
                                  int32_t K0, int32_t N1, int32_t N2, int32_t training, float slope, float bn_eps, float momentum, void* stream) {
    TG_REQUIRE(lh_shape_ok(B, K0, N1, N2, training), "tg_latent_head_fwd: (B, K0, N1, N2) = (%d, %d, %d, %d)%s is outside the envelope "
               "(1 <= B <= 512, B >= 2 in train mode, K0 <= 384, N1 <= 256, N2 <= 64)", B, K0, N1, N2, training ? " in train mode" : "");
    TG_REQUIRE(x && W1 && b1 && gamma && beta && running_mean && running_var && W2 && b2 && out && h1 && act_ws && stats, "tg_latent_head_fwd: null pointer");
    TG_REQUIRE(ldx >= K0 && ldo >= N2, "tg_latent_head_fwd: row strides below the row widths");
    const bool tail = Wmu != nullptr;
    TG_REQUIRE(!tail || (bmu && Wlv && blv && eps && h2 && mu && logvar), "tg_latent_head_fwd: the variational tail needs all of its operands");
    LhFwd a{x, (long)ldx, W1, b1, gamma, beta, running_mean, running_var, nbt, W2, b2, Wmu, bmu, Wlv, blv, eps, tail ? rng_state : nullptr, site,
            out, (long)ldo, h1, act_ws, stats, h2, mu, logvar, B, K0, N1, N2, training, slope, bn_eps, momentum};
    hipLaunchKernelGGL(latent_head_fwd_kernel, dim3(1), dim3(LH_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tg_latent_head_fwd");
}

extern "C" int tg_latent_head_bwd(const float* dout, int64_t ldo, const float* dmu, const float* dlv, const float* x, int64_t ldx, const float* W1,
                                  const float* gamma, const float* beta, const float* W2, const float* Wmu, const float* Wlv, const float* eps,
                                  const float* h1, const double* stats, const float* h2, const float* logvar, float* ws, float* dW1, float* db1,
                                  float* dgamma, float* dbeta, float* dW2, float* db2, float* dWmu, float* dbmu, float* dWlv, float* dblv, float* dx,
                                  int64_t lddx, int32_t B, int32_t K0, int32_t N1, int32_t N2, int32_t training, float slope, void* stream) {
    TG_REQUIRE(lh_shape_ok(B, K0, N1, N2, training), "tg_latent_head_bwd: (B, K0, N1, N2) = (%d, %d, %d, %d)%s is outside the envelope "
               "(1 <= B <= 512, B >= 2 in train mode, K0 <= 384, N1 <= 256, N2 <= 64)", B, K0, N1, N2, training ? " in train mode" : "");
    TG_REQUIRE(dout && x && W1 && gamma && beta && W2 && h1 && stats && ws && dW1 && db1 && dgamma && dbeta && dW2 && db2, "tg_latent_head_bwd: null pointer");
    TG_REQUIRE(ldx >= K0 && ldo >= N2 && (!dx || lddx >= K0), "tg_latent_head_bwd: row strides below the row widths");
    const bool tail = Wmu != nullptr;
    TG_REQUIRE(!tail || (Wlv && eps && h2 && logvar && dWmu && dbmu && dWlv && dblv), "tg_latent_head_bwd: the variational tail needs all of its operands");
    LhBwd a{dout, (long)ldo, tail ? dmu : nullptr, tail ? dlv : nullptr, x, (long)ldx, W1, gamma, beta, W2, Wmu, Wlv, eps, h1, stats, h2, logvar, ws,
            dW1, db1, dgamma, dbeta, dW2, db2, dWmu, dbmu, dWlv, dblv, dx, (long)lddx, B, K0, N1, N2, training, slope};
    hipLaunchKernelGGL(latent_head_bwd_kernel, dim3(1), dim3(LH_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tg_latent_head_bwd");
}
