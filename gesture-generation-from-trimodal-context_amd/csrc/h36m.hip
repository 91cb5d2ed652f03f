// Autoencoder batches from raw Human3.6M positions (data_loader/h36m_loader.py:16-17, :37-42, :44-64, :69-106, utils/data_utils.py:77-120): the
// arithmetic between data_3d_h36m.npz and the (target_poses, target_vec) batches of the FGD autoencoder, for many actions packed into one device
// buffer -- one launch per stage and batch, never one per action or window.
//
// h36m_normalize_kernel -- chunks of 128 frames: the 36 wanted floats of every frame (twelve joints; runs of 3 to 12 consecutive floats, read by
//   consecutive threads) go through LDS (rows padded to 37 floats: conflict-free per-frame reads), thread f owns frame f of the chunk: root
//   subtraction and axis swap in fp32, the frontalising angle and rotation in fp64, the 30 results back into the thread's own LDS row, stored coalesced.
// h36m_samples_kernel   -- one 128-thread workgroup per window, the layout of pp_windows_kernel (preprocess.hip): chunks of 128 frames through LDS
//   (coalesced load of the strided rows; rows padded to 31 floats), thread f owns frame f: direction vectors, rebuilt joints, noise (none, read, or
//   drawn from the library's Philox streams), direction vectors again minus the mean; both outputs staged in LDS and stored coalesced.
//
// Per-thread fp64 arithmetic without fused multiply-adds (-ffp-contract=off), no reductions, no atomics: bitwise repeatable.  The window table is
// device memory the host cannot inspect, so the samples kernel checks every entry against the extents it was given and flags (-1) instead of reading
// or writing outside.
#include "common.hpp"

#include <math.h>

namespace tg {

constexpr int HM_D = 30, HM_V = 27, HM_G = 36, HM_GROW = HM_G + 1, HM_ROW = HM_D + 1, HM_THREADS = 128, HM_MIN_JOINTS = 28;

// h36m_loader.py:17 target_joints as float offsets into a frame, one per gathered coordinate
__device__ const int hm_src[HM_G] = {3,  4,  5,  18, 19, 20, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47,
                                     51, 52, 53, 54, 55, 56, 57, 58, 59, 75, 76, 77, 78, 79, 80, 81, 82, 83};

// utils/data_utils.py:14-15 dir_vec_pairs as (bone, joint a, joint b, length): literal indices keep the frame in registers
#define HM_FOR_BONES(F) \
    F(0, 0, 1, 0.26) F(1, 1, 2, 0.18) F(2, 2, 3, 0.14) F(3, 1, 4, 0.22) F(4, 4, 5, 0.36) F(5, 5, 6, 0.33) F(6, 1, 7, 0.22) F(7, 7, 8, 0.36) F(8, 8, 9, 0.33)

__global__ __launch_bounds__(HM_THREADS) void h36m_normalize_kernel(const float* __restrict__ pos, long rows, int row_floats, float* __restrict__ out) {
    __shared__ float fr[HM_THREADS * HM_GROW];
    const int t = threadIdx.x;
    for (long f0 = (long)blockIdx.x * HM_THREADS; f0 < rows; f0 += (long)gridDim.x * HM_THREADS) {
        const int nf = rows - f0 < HM_THREADS ? (int)(rows - f0) : HM_THREADS;
        __syncthreads();                                      // (the previous chunk's LDS reads done)
        for (int e = t; e < nf * HM_G; e += HM_THREADS) {
            const int f = e / HM_G, k = e - f * HM_G;
            fr[f * HM_GROW + k] = pos[(f0 + f) * row_floats + hm_src[k]];
        }
        __syncthreads();
        if (t < nf) {
            float* __restrict__ me = fr + t * HM_GROW;
            // :73-75 in fp32, as numpy does on the fp32 array: minus gathered joint 2, then (x, y, z) -> (x, -z, y)
            const float rx = me[6], ry = me[7], rz = me[8];
            float x[12], y[12], z[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                x[j] = me[3 * j] - rx;
                y[j] = -(me[3 * j + 2] - rz);
                z[j] = me[3 * j + 1] - ry;
            }
            // :79-84: the hip vector in fp32, the angle in fp64; the wrap exactly as written (0, 180 and 360 degrees fall through both tests)
            const float hx = x[1] - x[0], hz = z[1] - z[0];
            const double pi = 3.141592653589793;
            double angle = pi - atan2((double)hz, (double)hx);
            const double deg = angle * (180.0 / pi);
            if (180.0 > deg && deg > 0.0) {
            } else if (180.0 < deg && deg < 360.0) {
                angle = angle - 360.0 * (pi / 180.0);
            }
            // :93-106 about (0, 1, 0): b = d = 0, c = -sin(angle / 2)
            const double a = cos(angle / 2.0), c = -sin(angle / 2.0);
            const double aa = a * a, cc = c * c, ac = a * c;
            const double r00 = aa - cc, r02 = 2.0 * (0.0 - ac), r11 = aa + cc, r20 = 2.0 * (0.0 + ac), r22 = aa - cc;
            // :87, :89: row vector @ matrix, products added left to right, one rounding; joints 0 and 1 dropped
#pragma unroll
            for (int j = 2; j < 12; ++j) {
                const double px = (double)x[j], py = (double)y[j], pz = (double)z[j];
                me[3 * (j - 2)] = (float)(px * r00 + py * 0.0 + pz * r20);
                me[3 * (j - 2) + 1] = (float)(px * 0.0 + py * r11 + pz * 0.0);
                me[3 * (j - 2) + 2] = (float)(px * r02 + py * 0.0 + pz * r22);
            }
        }
        __syncthreads();
        for (int e = t; e < nf * HM_D; e += HM_THREADS) out[f0 * HM_D + e] = fr[(e / HM_D) * HM_GROW + e % HM_D];
    }
}

// the four floats normal_kernel (elementwise.hip) writes at indices 4 idx4 .. 4 idx4 + 3 for this state and site, bit for bit.  That file is
// compiled with the default contraction, this one without: the compiler expands log inline (log2 times ln 2 in two parts) and fuses the last
// multiply-add only where the CALL carries the contraction flag -- which the header's logf() wrapper takes from the command line.  So the
// logarithm is called as the builtin under a local contraction pragma: the same instructions as in normal_kernel (compared in the ISA; the
// bit-for-bit test of drawn against given noise guards it).  Nothing else here has a multiply followed by an add.
__device__ __forceinline__ void hm_normal4(const uint64_t* __restrict__ st, uint32_t site, uint64_t idx4, float (&z)[4]) {
#pragma clang fp contract(fast)
    uint32_t r[4];
    philox4x32(st[0], idx4, site, (uint32_t)st[1], r);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const float rad = sqrtf(-2.f * __builtin_logf(u01(r[2 * q])));
        const float ang = 6.283185307179586f * u01(r[2 * q + 1]);
        z[2 * q] = rad * cosf(ang);
        z[2 * q + 1] = rad * sinf(ang);
    }
}

// NOISE: 0 none, 1 read from `noise`, 2 drawn
template <int NOISE>
__global__ __launch_bounds__(HM_THREADS) void h36m_samples_kernel(const float* __restrict__ skel, long skel_rows, const long* __restrict__ win_row0,
                                                                  int n_poses, int stride, const double* __restrict__ mean,
                                                                  const double* __restrict__ noise, const uint64_t* __restrict__ st, uint32_t noise_site,
                                                                  uint32_t select_site, float p_large, float std_large, float std_small,
                                                                  float* __restrict__ poses, float* __restrict__ vec, int* __restrict__ flag) {
    __shared__ float fr[HM_THREADS * HM_ROW];
    __shared__ float vst[HM_THREADS * HM_V];
    const int t = threadIdx.x, w = blockIdx.x;
    const long row0 = win_row0[w];
    const long span = (long)(n_poses - 1) * stride;           // (n_poses, stride <= 2^20: no overflow; extents compared by subtraction)
    if (row0 < 0 || span > skel_rows - 1 || row0 > skel_rows - 1 - span) {       // a table entry outside the buffer: nothing is read or written
        if (t == 0) flag[w] = -1;
        return;
    }
    if (t == 0) flag[w] = 0;
    double sd = 0.0;
    if (NOISE == 2) {                                         // element w of tg_dropout_mask(.., p_large, st, select_site) is 0 <=> u01 < p_large
        uint32_t r[4];
        philox4x32(st[0], (uint64_t)(w >> 2), select_site, (uint32_t)st[1], r);
        const uint32_t rw = (w & 3) == 0 ? r[0] : ((w & 3) == 1 ? r[1] : ((w & 3) == 2 ? r[2] : r[3]));
        sd = (double)(u01(rw) >= p_large ? std_small : std_large);
    }
    for (int f0 = 0; f0 < n_poses; f0 += HM_THREADS) {
        const int nf = n_poses - f0 < HM_THREADS ? n_poses - f0 : HM_THREADS;
        __syncthreads();                                      // (the previous chunk's LDS reads done)
        for (int e = t; e < nf * HM_D; e += HM_THREADS) {
            const int f = e / HM_D, c = e - f * HM_D;
            fr[f * HM_ROW + c] = skel[(row0 + (long)(f0 + f) * stride) * HM_D + c];
        }
        __syncthreads();
        if (t < nf) {
            float* __restrict__ me = fr + t * HM_ROW;
            float x[HM_D];
            double p[HM_D];
#pragma unroll
            for (int q = 0; q < HM_D; ++q) x[q] = me[q];
            p[0] = 0.0; p[1] = 0.0; p[2] = 0.0;
            // data_utils.py:101-109 then :77-98: fp32 differences, fp64 unit vectors (zero-length bone: zeros), joints from the bone lengths
#define HM_BONE(b, ja, jb, len)                                                                                              \
    {                                                                                                                        \
        const float fx = x[3 * jb] - x[3 * ja], fy = x[3 * jb + 1] - x[3 * ja + 1], fz = x[3 * jb + 2] - x[3 * ja + 2];      \
        const double dx = (double)fx, dy = (double)fy, dz = (double)fz;                                                      \
        double n = sqrt(dx * dx + dy * dy + dz * dz);                                                                        \
        n = n == 0.0 ? 1.0 : n;                                                                                              \
        p[3 * jb] = p[3 * ja] + len * (dx / n);                                                                              \
        p[3 * jb + 1] = p[3 * ja + 1] + len * (dy / n);                                                                      \
        p[3 * jb + 2] = p[3 * ja + 2] + len * (dz / n);                                                                      \
    }
            HM_FOR_BONES(HM_BONE)
#undef HM_BONE
            const long base = ((long)w * n_poses + f0 + t) * HM_D;
            if (NOISE == 1) {                                 // h36m_loader.py:49-56 with the final additive values given (tests replay recorded draws)
#pragma unroll
                for (int q = 0; q < HM_D; ++q) p[q] += noise[base + q];
            }
            if (NOISE == 2) {                                 // elements base .. base + 29 of tg_normal(.., st, noise_site): base is even, 8 Philox draws
                float z[32];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    float z4[4];
                    hm_normal4(st, noise_site, (uint64_t)(base >> 2) + g, z4);
                    z[4 * g] = z4[0]; z[4 * g + 1] = z4[1]; z[4 * g + 2] = z4[2]; z[4 * g + 3] = z4[3];
                }
                const bool odd = (base & 2) != 0;             // base % 4 is 0 or 2
#pragma unroll
                for (int q = 0; q < HM_D; ++q) p[q] += (double)(odd ? z[q + 2] : z[q]) * sd;
            }
            // :58-60: unit vectors of the (noisy) fp64 joints, minus the data mean
#define HM_BONE(b, ja, jb, len)                                                                                              \
    {                                                                                                                        \
        const double dx = p[3 * jb] - p[3 * ja], dy = p[3 * jb + 1] - p[3 * ja + 1], dz = p[3 * jb + 2] - p[3 * ja + 2];     \
        double n = sqrt(dx * dx + dy * dy + dz * dz);                                                                        \
        n = n == 0.0 ? 1.0 : n;                                                                                              \
        vst[t * HM_V + 3 * b] = (float)(dx / n - mean[3 * b]);                                                               \
        vst[t * HM_V + 3 * b + 1] = (float)(dy / n - mean[3 * b + 1]);                                                       \
        vst[t * HM_V + 3 * b + 2] = (float)(dz / n - mean[3 * b + 2]);                                                       \
    }
            HM_FOR_BONES(HM_BONE)
#undef HM_BONE
#pragma unroll
            for (int q = 0; q < HM_D; ++q) me[q] = (float)p[q];
        }
        __syncthreads();
        const long o = (long)w * n_poses + f0;
        for (int e = t; e < nf * HM_D; e += HM_THREADS) poses[o * HM_D + e] = fr[(e / HM_D) * HM_ROW + e % HM_D];
        for (int e = t; e < nf * HM_V; e += HM_THREADS) vec[o * HM_V + e] = vst[e];
    }
}

}  // namespace tg

using namespace tg;

#define HM_MAX_ROWS ((int64_t)1 << 40)

extern "C" int tg_h36m_normalize(const float* positions, int64_t rows, int32_t n_joints, float* out, void* stream) {
    TG_REQUIRE(positions && out, "tg_h36m_normalize: NULL pointer argument (positions, out)");
    TG_REQUIRE(rows >= 1 && rows < HM_MAX_ROWS, "tg_h36m_normalize: rows = %lld must be positive", (long long)rows);
    TG_REQUIRE(n_joints >= HM_MIN_JOINTS && n_joints <= 65536, "tg_h36m_normalize: n_joints = %d, at least %d needed (target_joints reach joint 27)",
               (int)n_joints, HM_MIN_JOINTS);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(positions) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0,
               "tg_h36m_normalize: misaligned pointer (positions, out: 4 bytes)");
    int64_t grid = (rows + HM_THREADS - 1) / HM_THREADS;
    grid = grid > 4096 ? 4096 : grid;
    hipLaunchKernelGGL(h36m_normalize_kernel, dim3((unsigned)grid), dim3(HM_THREADS), 0, (hipStream_t)stream, positions, (long)rows, (int)n_joints * 3, out);
    return check_launch("tg_h36m_normalize");
}

extern "C" int tg_h36m_samples(const float* skel, int64_t skel_rows, const void* win_row0, int64_t table_bytes, int32_t n_windows, int32_t n_poses,
                               int32_t frame_stride, const void* mean_dir_vec, int64_t mean_bytes, const void* noise, int64_t noise_bytes,
                               const uint64_t* rng_state, uint32_t noise_site, uint32_t select_site, float p_large, float std_large, float std_small,
                               float* poses, float* vec, int32_t* flag, void* stream) {
    TG_REQUIRE(skel && win_row0 && mean_dir_vec && poses && vec && flag, "tg_h36m_samples: NULL pointer argument (skel, win_row0, mean_dir_vec, poses, vec, flag)");
    TG_REQUIRE(n_windows >= 1 && n_poses >= 1 && n_poses <= (1 << 20) && frame_stride >= 1 && frame_stride <= (1 << 20),
               "tg_h36m_samples: n_windows = %d (>= 1), n_poses = %d, frame_stride = %d (1 .. 2^20)", (int)n_windows, (int)n_poses, (int)frame_stride);
    TG_REQUIRE(skel_rows >= 1 && skel_rows < HM_MAX_ROWS, "tg_h36m_samples: skel_rows = %lld must be positive", (long long)skel_rows);
    TG_REQUIRE(table_bytes >= (int64_t)n_windows * 8, "tg_h36m_samples: window table of %lld bytes, %lld needed", (long long)table_bytes,
               (long long)n_windows * 8);
    TG_REQUIRE(mean_bytes >= (int64_t)HM_V * 8, "tg_h36m_samples: mean_dir_vec of %lld bytes, %d needed (27 doubles)", (long long)mean_bytes, HM_V * 8);
    TG_REQUIRE(!(noise && rng_state), "tg_h36m_samples: noise and rng_state are both given (read the noise or draw it, not both)");
    const int64_t noise_need = (int64_t)n_windows * n_poses * HM_D * 8;
    TG_REQUIRE(!noise || noise_bytes >= noise_need, "tg_h36m_samples: noise of %lld bytes, %lld needed (n_windows x n_poses x 30 doubles)",
               (long long)noise_bytes, (long long)noise_need);
    TG_REQUIRE(!rng_state || (p_large >= 0.f && p_large < 1.f && std_large >= 0.f && std_small >= 0.f),
               "tg_h36m_samples: p_large = %g (0 <= p < 1), std_large = %g, std_small = %g (>= 0)", (double)p_large, (double)std_large, (double)std_small);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(win_row0) & 7u) == 0 && (reinterpret_cast<uintptr_t>(mean_dir_vec) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(noise) & 7u) == 0 && (reinterpret_cast<uintptr_t>(rng_state) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(skel) & 3u) == 0 && (reinterpret_cast<uintptr_t>(poses) & 3u) == 0 &&
               (reinterpret_cast<uintptr_t>(vec) & 3u) == 0 && (reinterpret_cast<uintptr_t>(flag) & 3u) == 0,
               "tg_h36m_samples: misaligned pointer (win_row0, mean_dir_vec, noise, rng_state: 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)n_windows), block(HM_THREADS);
    const long* tab = static_cast<const long*>(win_row0);
    const double* mean = static_cast<const double*>(mean_dir_vec);
    const double* nz = static_cast<const double*>(noise);
    if (rng_state)
        hipLaunchKernelGGL(h36m_samples_kernel<2>, grid, block, 0, s, skel, (long)skel_rows, tab, (int)n_poses, (int)frame_stride, mean, nz, rng_state,
                           noise_site, select_site, p_large, std_large, std_small, poses, vec, (int*)flag);
    else if (noise)
        hipLaunchKernelGGL(h36m_samples_kernel<1>, grid, block, 0, s, skel, (long)skel_rows, tab, (int)n_poses, (int)frame_stride, mean, nz, rng_state,
                           noise_site, select_site, p_large, std_large, std_small, poses, vec, (int*)flag);
    else
        hipLaunchKernelGGL(h36m_samples_kernel<0>, grid, block, 0, s, skel, (long)skel_rows, tab, (int)n_poses, (int)frame_stride, mean, nz, rng_state,
                           noise_site, select_site, p_large, std_large, std_small, poses, vec, (int*)flag);
    return check_launch("tg_h36m_samples");
}
