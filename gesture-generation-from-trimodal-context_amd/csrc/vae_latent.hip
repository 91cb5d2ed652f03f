// Variational tail of the pose encoder (model/embedding_net.py:67-82 with variational_encoding=True, the KL term of
// train_feature_extractor.py:74-79 / train_eval/train_joint_embed.py:30-36): f3 [B][32] -> mu = fc_mu(f3), logvar = fc_logvar(f3),
// z = mu + eps exp(logvar / 2) and KLD = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) over the whole batch, ONE launch each way.
//
// Organisation: ONE workgroup of 512 threads = 16 row groups x 32 columns; a thread owns one column and the rows g, g + 16, g + 32, ..
// The work is 2 x 32 x 32 multiply-adds per row -- microseconds at the envelope's edge, latency at the batch sizes that train -- so a grid
// would buy nothing and cost a device-wide hand-off for the KL sum and the weight gradients.  Both 32 x 32 weight matrices sit in LDS
// (forward: transposed, [k][c], so the 32 lanes of a row group read 32 consecutive words; backward: as stored, [c][k], for df3); the rows of
// f3 / dmu / dlv are read from global memory with one address per row group (a broadcast).  Every dot product and every sum over the batch is
// ONE fp64 chain in ascending index order, rounded to fp32 once: row b of mu / logvar / z depends on row b of the inputs only and its bits do
// not change with B, and two runs are bit identical (no atomics).  The KL terms are formed in fp64 from the fp32 mu / logvar just written:
// per-thread partial sums over the thread's rows in ascending order, then a fixed halving tree over the 512 partials in LDS.
// The backward keeps dmu / dlv [B][32] in a caller-provided workspace (written and read by this one workgroup, a barrier in between).
#include "common.hpp"

namespace tg {
namespace {

constexpr int VL_THREADS = 512;
constexpr int VL_N = 32;                    // latent width (fc_mu / fc_logvar are 32 x 32)
constexpr int VL_GROUPS = VL_THREADS / VL_N;
constexpr int VL_MAX_B = 1024;

// sum of the 512 per-thread values in a fixed order (halving tree); the result is returned to every thread
__device__ double vl_block_sum(double* red, double v) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = VL_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// element i of tg_normal(eps, n, state, site), bit for bit (as csrc/latent_head.hip, csrc/speaker.hip)
__device__ __forceinline__ float vl_normal(const uint64_t* rng, uint32_t site, int i) {
    uint32_t r[4];
    philox4x32(rng[0], (uint64_t)(i >> 2), site, (uint32_t)rng[1], r);
    const int q = (i & 3) >> 1;
    const float rad = sqrtf(-2.f * logf(u01(r[2 * q])));
    const float ang = 6.283185307179586f * u01(r[2 * q + 1]);
    return (i & 1) ? rad * sinf(ang) : rad * cosf(ang);
}

__device__ __forceinline__ double vl_kl_term(float mu, float logvar) {
    const double m = (double)mu, l = (double)logvar;
    return 1.0 + l - m * m - exp(l);
}

struct VlFwd {
    const float *f3, *Wmu, *bmu, *Wlv, *blv;
    float* eps; const uint64_t* rng; uint32_t site;
    float *mu, *logvar, *z; double* kld;
    int B;
};

__global__ __launch_bounds__(VL_THREADS) void vae_latent_fwd_kernel(VlFwd a) {
    __shared__ float wm[VL_N][VL_N + 1], wl[VL_N][VL_N + 1];          // [k][c]
    __shared__ double red[VL_THREADS];
    const int t = threadIdx.x, c = t % VL_N, g = t / VL_N, B = a.B;
    for (int i = t; i < VL_N * VL_N; i += VL_THREADS) {
        wm[i % VL_N][i / VL_N] = a.Wmu[i];
        wl[i % VL_N][i / VL_N] = a.Wlv[i];
    }
    __syncthreads();
    const double bm = (double)a.bmu[c], bl = (double)a.blv[c];
    double part = 0.0;
    for (int b = g; b < B; b += VL_GROUPS) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(a.f3 + (long)b * VL_N);
        double sm = 0.0, sl = 0.0;
#pragma unroll
        for (int q = 0; q < VL_N / 4; ++q) {
            const f32x4 xv = x4[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sm = fma((double)xv[j], (double)wm[4 * q + j][c], sm);
                sl = fma((double)xv[j], (double)wl[4 * q + j][c], sl);
            }
        }
        const float mu = (float)(sm + bm), lv = (float)(sl + bl);
        const int i = b * VL_N + c;
        float e;
        if (a.rng) {
            e = vl_normal(a.rng, a.site, i);
            a.eps[i] = e;
        } else {
            e = a.eps[i];
        }
        a.mu[i] = mu;
        a.logvar[i] = lv;
        a.z[i] = mu + e * expf(0.5f * lv);
        part += vl_kl_term(mu, lv);
    }
    const double total = vl_block_sum(red, part);
    if (t == 0) *a.kld = -0.5 * total;
}

struct VlBwd {
    const float *dz, *dmu_in, *dlv_in, *mu, *logvar, *eps, *f3, *Wmu, *Wlv;
    float w;
    float* ws;
    float *dWmu, *dbmu, *dWlv, *dblv, *df3;
    int B;
};

__global__ __launch_bounds__(VL_THREADS) void vae_latent_bwd_kernel(VlBwd a) {
    __shared__ float wm[VL_N][VL_N], wl[VL_N][VL_N];                  // [c][k], as stored
    const int t = threadIdx.x, k = t % VL_N, g = t / VL_N, B = a.B;
    float* dm = a.ws;                       // [B][32]
    float* dl = a.ws + (long)B * VL_N;      // [B][32]
    for (int i = t; i < VL_N * VL_N; i += VL_THREADS) {
        wm[i / VL_N][i % VL_N] = a.Wmu[i];
        wl[i / VL_N][i % VL_N] = a.Wlv[i];
    }
    for (int i = t; i < B * VL_N; i += VL_THREADS) {
        const float lv = a.logvar[i];
        float m = a.w * a.mu[i], l = a.w * 0.5f * (expf(lv) - 1.f);
        if (a.dz) {
            const float dz = a.dz[i];
            m = dz + m;
            l = dz * a.eps[i] * 0.5f * expf(0.5f * lv) + l;
        }
        if (a.dmu_in) m += a.dmu_in[i];
        if (a.dlv_in) l += a.dlv_in[i];
        dm[i] = m;
        dl[i] = l;
    }
    __syncthreads();
    // weight and bias gradients: 2 x 32 x 32 outputs, four per thread, each one fp64 chain over the rows in ascending order
    for (int pass = 0; pass < 2 * VL_N / VL_GROUPS; ++pass) {
        const int o = pass * VL_GROUPS + g, mat = o / VL_N, c = o % VL_N;
        const float* d = mat ? dl : dm;
        double sw = 0.0, sb = 0.0;
        for (int b = 0; b < B; ++b) {
            const double dv = (double)d[(long)b * VL_N + c];
            sw = fma(dv, (double)a.f3[(long)b * VL_N + k], sw);
            sb += dv;
        }
        (mat ? a.dWlv : a.dWmu)[c * VL_N + k] = (float)sw;
        if (k == 0) (mat ? a.dblv : a.dbmu)[c] = (float)sb;
    }
    // df3[b][k] = sum_c dmu[b][c] Wmu[c][k] + sum_c dlv[b][c] Wlv[c][k]
    for (int b = g; b < B; b += VL_GROUPS) {
        const f32x4* m4 = reinterpret_cast<const f32x4*>(dm + (long)b * VL_N);
        const f32x4* l4 = reinterpret_cast<const f32x4*>(dl + (long)b * VL_N);
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < VL_N / 4; ++q) {
            const f32x4 v = m4[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fma((double)v[j], (double)wm[4 * q + j][k], s);
        }
#pragma unroll
        for (int q = 0; q < VL_N / 4; ++q) {
            const f32x4 v = l4[q];
#pragma unroll
            for (int j = 0; j < 4; ++j) s = fma((double)v[j], (double)wl[4 * q + j][k], s);
        }
        a.df3[(long)b * VL_N + k] = (float)s;
    }
}

// KL term of a latent whose head runs elsewhere (the context encoder's): value and gradient, one launch
__global__ __launch_bounds__(VL_THREADS) void vae_kld_kernel(const float* mu, const float* logvar, int n, float w, double* kld, float* dmu,
                                                            float* dlv) {
    __shared__ double red[VL_THREADS];
    const int t = threadIdx.x;
    double part = 0.0;
    for (int i = t; i < n; i += VL_THREADS) {
        const float m = mu[i], l = logvar[i];
        part += vl_kl_term(m, l);
        if (dmu) {
            dmu[i] = w * m;
            dlv[i] = w * 0.5f * (expf(l) - 1.f);
        }
    }
    const double total = vl_block_sum(red, part);
    if (t == 0) *kld = -0.5 * total;
}

}  // namespace
}  // namespace tg

using namespace tg;

extern "C" int tg_vae_latent_fwd(const float* f3, const float* Wmu, const float* bmu, const float* Wlv, const float* blv, float* eps,
                                 const uint64_t* rng_state, uint32_t site, float* mu, float* logvar, float* z, double* kld, int32_t B,
                                 void* stream) {
    TG_REQUIRE(B >= 1 && B <= VL_MAX_B, "tg_vae_latent_fwd: B = %d is outside the envelope (1 <= B <= 1024)", B);
    TG_REQUIRE(f3 && Wmu && bmu && Wlv && blv && eps && mu && logvar && z && kld, "tg_vae_latent_fwd: null pointer");
    VlFwd a{f3, Wmu, bmu, Wlv, blv, eps, rng_state, site, mu, logvar, z, kld, B};
    hipLaunchKernelGGL(vae_latent_fwd_kernel, dim3(1), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tg_vae_latent_fwd");
}

extern "C" int tg_vae_latent_bwd(const float* dz, const float* dmu, const float* dlv, const float* mu, const float* logvar, const float* eps,
                                 const float* f3, const float* Wmu, const float* Wlv, float w, float* ws, float* dWmu, float* dbmu, float* dWlv,
                                 float* dblv, float* df3, int32_t B, void* stream) {
    TG_REQUIRE(B >= 1 && B <= VL_MAX_B, "tg_vae_latent_bwd: B = %d is outside the envelope (1 <= B <= 1024)", B);
    TG_REQUIRE(mu && logvar && f3 && Wmu && Wlv && ws && dWmu && dbmu && dWlv && dblv && df3, "tg_vae_latent_bwd: null pointer");
    TG_REQUIRE(!dz || eps, "tg_vae_latent_bwd: dz needs the forward's eps");
    VlBwd a{dz, dmu, dlv, mu, logvar, eps, f3, Wmu, Wlv, w, ws, dWmu, dbmu, dWlv, dblv, df3, B};
    hipLaunchKernelGGL(vae_latent_bwd_kernel, dim3(1), dim3(VL_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("tg_vae_latent_bwd");
}

extern "C" int tg_vae_kld(const float* mu, const float* logvar, int32_t B, int32_t N, float w, double* kld, float* dmu, float* dlv, void* stream) {
    TG_REQUIRE(B >= 1 && N >= 1 && (int64_t)B * N <= (int64_t)VL_MAX_B * 64, "tg_vae_kld: (B, N) = (%d, %d) is outside the envelope (B N <= 65536)", B, N);
    TG_REQUIRE(mu && logvar && kld && (dmu == nullptr) == (dlv == nullptr), "tg_vae_kld: null pointer (dmu / dlv go together)");
    hipLaunchKernelGGL(vae_kld_kernel, dim3(1), dim3(VL_THREADS), 0, (hipStream_t)stream, mu, logvar, B * N, w, kld, dmu, dlv);
    return check_launch("tg_vae_kld");
}
