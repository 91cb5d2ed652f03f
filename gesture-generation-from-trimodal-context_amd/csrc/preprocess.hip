// Training samples from raw clips (data_loader/data_preprocessor.py:66-170, data_loader/motion_preprocessor.py:32-87, utils/data_utils.py:46-56,
// data_loader/calculate_motion_stats.py:33-44): the arithmetic between the clip store and the sample store, for a BATCH of clips packed into one
// device buffer and described by device-resident tables -- one launch per stage and batch, never one per clip or window.
//
// pp_resample_kernel  -- element-parallel over the (frame, coordinate) pairs of every clip's output (consecutive threads read consecutive floats
//   of a frame); the owning clip is found by bisection of the clip table; position k * step and the interpolation in fp64.
// pp_windows_kernel   -- one 128-thread workgroup per window: chunks of 128 frames go through LDS (coalesced load, pose copy on the way; rows
//   padded to 31 floats: conflict-free per-frame reads), thread f owns frame f of the chunk: spine angle, nine direction vectors (staged in LDS,
//   stored coalesced), |x - mean_pose|, wrist moments.  fp64 accumulators per thread, xor-butterfly wave reductions in registers, one LDS step
//   over the two waves in wave order: a fixed order, no atomics.
// pp_slices_kernel    -- one workgroup column per window: a gather with np.pad(mode = 'symmetric') index arithmetic (period 2 L).
// pp_stats_kernel     -- fp64 partial sums per workgroup (frames through LDS in chunks of 64, per-frame results in an LDS matrix, thread c sums
//   column c in frame order), pp_stats_final_kernel adds the partials in workgroup order.
//
// The tables are device memory the host cannot inspect, so every kernel checks what it reads from them against the buffer extents it was given
// and skips (windows: verdict -1) instead of reading or writing outside.
#include "common.hpp"

#include <math.h>

namespace tg {

constexpr int PP_D = 30, PP_V = 27, PP_BONES = 9, PP_STATS = 6;
constexpr int PP_CLIP_WORDS = 5;                  // tg_pose_resample clip record: src_row0, n, dst_row0, m (int64), step (double)
constexpr int PP_SLICE_WORDS = 4;                 // tg_clip_slices window record: base, L, row_stride, start (int64)
constexpr int PP_CONSTS = PP_D + PP_V + 4;        // mean_pose, mean_dir_vec, thresholds (pose, max angle, mean angle, variance)
constexpr int PP_WIN_THREADS = 128, PP_ROW = PP_D + 1;
constexpr int PP_ST_THREADS = 128, PP_ST_CHUNK = 64, PP_ST_COLS = PP_D + PP_V + PP_BONES, PP_ST_MAX_WG = 256;

// utils/data_utils.py:14-15 dir_vec_pairs as (bone, joint a, joint b): literal indices keep the frame's 30 values in registers
#define PP_FOR_BONES(F) F(0, 0, 1) F(1, 1, 2) F(2, 2, 3) F(3, 1, 4) F(4, 4, 5) F(5, 5, 6) F(6, 1, 7) F(7, 7, 8) F(8, 8, 9)

struct PpClip {
    long src_row0, n, dst_row0, m;
    double step;
};

__device__ __forceinline__ double pp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double pp_wave_max(double v) {                  // NaN-propagating, like Python's max over a list that starts with it
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double w = __shfl_xor(v, o, 64); v = (w > v || w != w) ? w : v; }
    return v;
}

template <typename T>
__global__ __launch_bounds__(256) void pp_resample_kernel(const T* __restrict__ src, long src_rows, const PpClip* __restrict__ clips, int n_clips,
                                                          T* __restrict__ dst, long dst_rows) {
    const long total = dst_rows * PP_D;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long r = e / PP_D;
        const int j = (int)(e - r * PP_D);
        int lo_c = 0, hi_c = n_clips - 1;                     // last clip whose dst_row0 <= r (the host packs outputs in clip order)
        while (lo_c < hi_c) {
            const int mid = (lo_c + hi_c + 1) >> 1;
            if (clips[mid].dst_row0 <= r) lo_c = mid; else hi_c = mid - 1;
        }
        const PpClip c = clips[lo_c];
        const long k = r - c.dst_row0;
        if (k < 0 || k >= c.m || c.n < 1 || c.src_row0 < 0 || c.n > src_rows || c.src_row0 > src_rows - c.n) continue;
        const T* __restrict__ y = src + c.src_row0 * PP_D + j;
        if (c.n < 2) { dst[e] = y[0]; continue; }
        // scipy.interpolate.interp1d(kind = 'linear', fill_value = 'extrapolate') on x = 0 .. n - 1: the segment is searchsorted(x, x_new) =
        // ceil(x_new) clipped to [1, n - 1]; the difference of the two samples is taken in THEIR dtype (numpy subtracts the fp32 / fp16 arrays),
        // everything after it in fp64: slope * (x_new - x_lo) + y_lo, rounded once to the input dtype
        const double x = (double)k * c.step;
        long hi = (long)ceil(x);
        hi = hi < 1 ? 1 : (hi > c.n - 1 ? c.n - 1 : hi);
        const long lo = hi - 1;
        const T y_lo = y[lo * PP_D], y_hi = y[hi * PP_D];
        const T d = y_hi - y_lo;
        dst[e] = (T)((double)d * (x - (double)lo) + (double)y_lo);
    }
}

template <typename T>
__global__ __launch_bounds__(PP_WIN_THREADS) void pp_windows_kernel(const T* __restrict__ skel, long skel_rows, const long* __restrict__ win_row0,
                                                                    int n_poses, const double* __restrict__ consts, T* __restrict__ poses,
                                                                    float* __restrict__ vec, float* __restrict__ stats, int* __restrict__ verdict) {
    __shared__ float fr[PP_WIN_THREADS * PP_ROW];
    __shared__ float vst[PP_WIN_THREADS * PP_V];
    __shared__ double first[PP_D];
    __shared__ double red[2][4], mom[2][12];
    const int t = threadIdx.x, w = blockIdx.x;
    const long row0 = win_row0[w];
    if (row0 < 0 || row0 > skel_rows - n_poses) {             // a table entry outside the buffer: nothing is read
        if (t == 0) verdict[w] = -1;
        return;
    }
    const T* __restrict__ in = skel + row0 * PP_D;
    if (t < PP_D) first[t] = (double)in[t];
    double abs_sum = 0.0, ang_sum = 0.0, ang_max = -1.0, bad = 0.0, s1[6] = {0, 0, 0, 0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};
    for (int f0 = 0; f0 < n_poses; f0 += PP_WIN_THREADS) {
        const int nf = n_poses - f0 < PP_WIN_THREADS ? n_poses - f0 : PP_WIN_THREADS;
        __syncthreads();                                      // (first[] written; the previous chunk's LDS reads done)
        for (int e = t; e < nf * PP_D; e += PP_WIN_THREADS) {
            const T v = in[(long)f0 * PP_D + e];
            poses[((long)w * n_poses + f0) * PP_D + e] = v;
            fr[(e / PP_D) * PP_ROW + e % PP_D] = (float)v;
        }
        __syncthreads();
        if (t < nf) {
            double x[PP_D];
#pragma unroll
            for (int q = 0; q < PP_D; ++q) {
                x[q] = (double)fr[t * PP_ROW + q];
                abs_sum += fabs(x[q] - consts[q]);
                bad += isfinite(x[q]) ? 0.0 : 1.0;
            }
            // motion_preprocessor.py:66-78: angle between joint 1 - joint 0 and (0, -1, 0)
            const double sx = x[3] - x[0], sy = x[4] - x[1], sz = x[5] - x[2];
            double c = -(sy / sqrt(sx * sx + sy * sy + sz * sz));
            c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
            const double ang = acos(c);
            ang_sum += ang;
            ang_max = (ang > ang_max || ang != ang) ? ang : ang_max;
            // :33-36: moments of joints 6 and 9 about the window's first frame (exact differences; a static window gives exactly zero)
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const int col = q < 3 ? 18 + q : 27 + q - 3;
                const double d = x[col] - first[col];
                s1[q] += d;
                s2[q] += d * d;
            }
            // utils/data_utils.py:101-109 + data_preprocessor.py:170: unit bone directions (zero-length bone: zeros) minus the data mean
#define PP_BONE(b, ja, jb)                                                                                                   \
    {                                                                                                                        \
        const double dx = x[3 * jb] - x[3 * ja], dy = x[3 * jb + 1] - x[3 * ja + 1], dz = x[3 * jb + 2] - x[3 * ja + 2];     \
        double n = sqrt(dx * dx + dy * dy + dz * dz);                                                                        \
        n = n == 0.0 ? 1.0 : n;                                                                                              \
        vst[t * PP_V + 3 * b] = (float)(dx / n - consts[PP_D + 3 * b]);                                                      \
        vst[t * PP_V + 3 * b + 1] = (float)(dy / n - consts[PP_D + 3 * b + 1]);                                              \
        vst[t * PP_V + 3 * b + 2] = (float)(dz / n - consts[PP_D + 3 * b + 2]);                                              \
    }
            PP_FOR_BONES(PP_BONE)
#undef PP_BONE
        }
        __syncthreads();
        for (int e = t; e < nf * PP_V; e += PP_WIN_THREADS) vec[((long)w * n_poses + f0) * PP_V + e] = vst[e];
    }
    // lanes without a frame hold the identities (0; -1 for the maximum of angles, which are >= 0)
    abs_sum = pp_wave_sum(abs_sum);
    ang_sum = pp_wave_sum(ang_sum);
    ang_max = pp_wave_max(ang_max);
    bad = pp_wave_sum(bad);
#pragma unroll
    for (int q = 0; q < 6; ++q) { s1[q] = pp_wave_sum(s1[q]); s2[q] = pp_wave_sum(s2[q]); }
    const int wave = t >> 6;
    if ((t & 63) == 0) {
        red[wave][0] = abs_sum; red[wave][1] = ang_sum; red[wave][2] = ang_max; red[wave][3] = bad;
#pragma unroll
        for (int q = 0; q < 6; ++q) { mom[wave][q] = s1[q]; mom[wave][6 + q] = s2[q]; }
    }
    __syncthreads();
    if (t == 0) {
        const double n = (double)n_poses;
        const double pose_diff = (red[0][0] + red[1][0]) / (n * PP_D);
        const double m1 = red[1][2];
        double mx = red[0][2];
        mx = (m1 > mx || m1 != m1) ? m1 : mx;
        const double rad2deg = 180.0 / 3.14159265358979323846;
        const double max_deg = mx * rad2deg, mean_deg = (red[0][1] + red[1][1]) / n * rad2deg;
        double var[2] = {0.0, 0.0};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double m = (mom[0][q] + mom[1][q]) / n;
            var[q / 3] += (mom[0][6 + q] + mom[1][6 + q]) / n - m * m;
        }
        const double n_bad = red[0][3] + red[1][3];
        const double* th = consts + PP_D + PP_V;
        int v = 0;                                            // motion_preprocessor.py:14-23: the first failing check wins
        if (pose_diff < th[0]) v = 1;
        else if (max_deg > th[1] || mean_deg > th[2]) v = 2;
        else if (var[0] < th[3] && var[1] < th[3]) v = 3;
        float* st = stats + (long)w * PP_STATS;
        st[0] = (float)pose_diff; st[1] = (float)max_deg; st[2] = (float)mean_deg; st[3] = (float)var[0]; st[4] = (float)var[1]; st[5] = (float)n_bad;
        verdict[w] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pp_slices_kernel(const T* __restrict__ src, long src_elems, int rows, const long* __restrict__ tab, int len,
                                                        T* __restrict__ dst) {
    const int w = blockIdx.x;
    const long base = tab[PP_SLICE_WORDS * w], L = tab[PP_SLICE_WORDS * w + 1], rs = tab[PP_SLICE_WORDS * w + 2], start = tab[PP_SLICE_WORDS * w + 3];
    const long total = (long)rows * len;
    // (extents compared by subtraction: no product or sum of table entries can overflow)
    const bool ok = L >= 1 && L <= src_elems && base >= 0 && base <= src_elems - L && rs >= 0 && start >= 0 &&
                    (rows == 1 || rs <= (src_elems - L - base) / (rows - 1));
    const long period = 2 * (ok ? L : 1), start_p = ok ? start % period : 0;      // start reduced first: start_p + j < 2 L + len
    for (long e = (long)blockIdx.y * 256 + threadIdx.x; e < total; e += (long)gridDim.y * 256) {
        const long r = e / len, j = e - r * len;
        // np.pad(mode = 'symmetric') past the end: ... x[L-2] x[L-1] | x[L-1] x[L-2] ... x[0] | x[0] x[1] ...: period 2 L
        long q = (start_p + j) % period;
        q = q < L ? q : 2 * L - 1 - q;
        dst[((long)w * rows + r) * len + j] = ok ? src[base + r * rs + q] : (T)0;
    }
}

template <typename T>
__global__ __launch_bounds__(PP_ST_THREADS) void pp_stats_kernel(const T* __restrict__ skel, long n_rows, double* __restrict__ partials) {
    __shared__ float fr[PP_ST_CHUNK * PP_ROW];
    __shared__ double res[PP_ST_CHUNK * (PP_ST_COLS + 1)];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (long f0 = (long)blockIdx.x * PP_ST_CHUNK; f0 < n_rows; f0 += (long)gridDim.x * PP_ST_CHUNK) {
        const int nf = n_rows - f0 < PP_ST_CHUNK ? (int)(n_rows - f0) : PP_ST_CHUNK;
        __syncthreads();
        for (int e = t; e < nf * PP_D; e += PP_ST_THREADS) fr[(e / PP_D) * PP_ROW + e % PP_D] = (float)skel[f0 * PP_D + e];
        __syncthreads();
        if (t < nf) {
            double x[PP_D];
            double* __restrict__ out = res + t * (PP_ST_COLS + 1);
#pragma unroll
            for (int q = 0; q < PP_D; ++q) { x[q] = (double)fr[t * PP_ROW + q]; out[q] = x[q]; }
#define PP_BONE(b, ja, jb)                                                                                                   \
    {                                                                                                                        \
        const double dx = x[3 * jb] - x[3 * ja], dy = x[3 * jb + 1] - x[3 * ja + 1], dz = x[3 * jb + 2] - x[3 * ja + 2];     \
        const double len = sqrt(dx * dx + dy * dy + dz * dz);                                                                \
        const double n = len == 0.0 ? 1.0 : len;                                                                             \
        out[PP_D + 3 * b] = dx / n; out[PP_D + 3 * b + 1] = dy / n; out[PP_D + 3 * b + 2] = dz / n;                          \
        out[PP_D + PP_V + b] = len;                                                                                          \
    }
            PP_FOR_BONES(PP_BONE)
#undef PP_BONE
        }
        __syncthreads();
        if (t < PP_ST_COLS)
            for (int f = 0; f < nf; ++f) acc += res[f * (PP_ST_COLS + 1) + t];
    }
    if (t < PP_ST_COLS) partials[(long)blockIdx.x * PP_ST_COLS + t] = acc;
}

__global__ __launch_bounds__(PP_ST_THREADS) void pp_stats_final_kernel(const double* __restrict__ partials, int n_wg, long n_rows, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= PP_ST_COLS) return;
    double acc = 0.0;
    for (int g = 0; g < n_wg; ++g) acc += partials[(long)g * PP_ST_COLS + t];
    out[t] = acc / (double)n_rows;
}

static int pp_stats_wgs(int64_t n_rows) {
    const int64_t g = (n_rows + PP_ST_CHUNK - 1) / PP_ST_CHUNK;
    return (int)(g < 1 ? 1 : (g > PP_ST_MAX_WG ? PP_ST_MAX_WG : g));
}

}  // namespace tg

using namespace tg;

#define PP_MAX_ROWS ((int64_t)1 << 40)

extern "C" int tg_pose_resample(const void* src, int64_t src_rows, int32_t half, const void* clips, int64_t clip_bytes, int32_t n_clips, void* dst,
                                int64_t dst_rows, void* stream) {
    TG_REQUIRE(src && clips && dst, "tg_pose_resample: NULL pointer argument");
    TG_REQUIRE(half == 0 || half == 1, "tg_pose_resample: half must be 0 (fp32) or 1 (fp16)");
    TG_REQUIRE(n_clips >= 1 && src_rows >= 1 && dst_rows >= 1 && src_rows < PP_MAX_ROWS && dst_rows < PP_MAX_ROWS,
               "tg_pose_resample: n_clips = %d, src_rows = %lld, dst_rows = %lld must be positive", (int)n_clips, (long long)src_rows, (long long)dst_rows);
    TG_REQUIRE(clip_bytes >= (int64_t)n_clips * PP_CLIP_WORDS * 8, "tg_pose_resample: clip table of %lld bytes, %lld needed (%d clips of 40 bytes)",
               (long long)clip_bytes, (long long)n_clips * PP_CLIP_WORDS * 8, (int)n_clips);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(clips) & 7u) == 0 && (reinterpret_cast<uintptr_t>(src) & (half ? 1u : 3u)) == 0 &&
               (reinterpret_cast<uintptr_t>(dst) & (half ? 1u : 3u)) == 0, "tg_pose_resample: misaligned pointer (table 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    const int grid = ew_grid(dst_rows * PP_D, 256, 2);
    if (half)
        hipLaunchKernelGGL(pp_resample_kernel<_Float16>, dim3(grid), dim3(256), 0, s, static_cast<const _Float16*>(src), (long)src_rows,
                           static_cast<const PpClip*>(clips), (int)n_clips, static_cast<_Float16*>(dst), (long)dst_rows);
    else
        hipLaunchKernelGGL(pp_resample_kernel<float>, dim3(grid), dim3(256), 0, s, static_cast<const float*>(src), (long)src_rows,
                           static_cast<const PpClip*>(clips), (int)n_clips, static_cast<float*>(dst), (long)dst_rows);
    return check_launch("tg_pose_resample");
}

extern "C" int tg_clip_windows(const void* skel, int64_t skel_rows, int32_t half, const void* win_row0, int64_t table_bytes, int32_t n_windows,
                               int32_t n_poses, const void* consts, int64_t const_bytes, void* poses, float* vec, float* stats, int32_t* verdict,
                               void* stream) {
    TG_REQUIRE(skel && win_row0 && consts && poses && vec && stats && verdict, "tg_clip_windows: NULL pointer argument");
    TG_REQUIRE(half == 0 || half == 1, "tg_clip_windows: half must be 0 (fp32) or 1 (fp16)");
    TG_REQUIRE(n_windows >= 1 && n_poses >= 1 && n_poses <= (1 << 20) && skel_rows >= n_poses && skel_rows < PP_MAX_ROWS,
               "tg_clip_windows: n_windows = %d, n_poses = %d (1 .. 2^20), skel_rows = %lld (>= n_poses)", (int)n_windows, (int)n_poses, (long long)skel_rows);
    TG_REQUIRE(table_bytes >= (int64_t)n_windows * 8, "tg_clip_windows: window table of %lld bytes, %lld needed", (long long)table_bytes, (long long)n_windows * 8);
    TG_REQUIRE(const_bytes >= (int64_t)PP_CONSTS * 8, "tg_clip_windows: constants of %lld bytes, %d needed (30 + 27 + 4 doubles)", (long long)const_bytes, PP_CONSTS * 8);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(win_row0) & 7u) == 0 && (reinterpret_cast<uintptr_t>(consts) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(skel) & (half ? 1u : 3u)) == 0 && (reinterpret_cast<uintptr_t>(poses) & (half ? 1u : 3u)) == 0 &&
               (reinterpret_cast<uintptr_t>(vec) & 3u) == 0 && (reinterpret_cast<uintptr_t>(stats) & 3u) == 0 && (reinterpret_cast<uintptr_t>(verdict) & 3u) == 0,
               "tg_clip_windows: misaligned pointer (tables 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (half)
        hipLaunchKernelGGL(pp_windows_kernel<_Float16>, dim3((unsigned)n_windows), dim3(PP_WIN_THREADS), 0, s, static_cast<const _Float16*>(skel),
                           (long)skel_rows, static_cast<const long*>(win_row0), (int)n_poses, static_cast<const double*>(consts),
                           static_cast<_Float16*>(poses), vec, stats, (int*)verdict);
    else
        hipLaunchKernelGGL(pp_windows_kernel<float>, dim3((unsigned)n_windows), dim3(PP_WIN_THREADS), 0, s, static_cast<const float*>(skel),
                           (long)skel_rows, static_cast<const long*>(win_row0), (int)n_poses, static_cast<const double*>(consts),
                           static_cast<float*>(poses), vec, stats, (int*)verdict);
    return check_launch("tg_clip_windows");
}

extern "C" int tg_clip_slices(const void* src, int64_t src_elems, int32_t elem_bytes, int32_t rows, const void* table, int64_t table_bytes,
                              int32_t n_windows, int32_t len, void* dst, void* stream) {
    TG_REQUIRE(src && table && dst, "tg_clip_slices: NULL pointer argument");
    TG_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "tg_clip_slices: elem_bytes = %d, 2 or 4 supported", (int)elem_bytes);
    TG_REQUIRE(n_windows >= 1 && rows >= 1 && rows <= 65535 && len >= 1 && src_elems >= 1 && src_elems < PP_MAX_ROWS,
               "tg_clip_slices: n_windows = %d, rows = %d, len = %d, src_elems = %lld must be positive", (int)n_windows, (int)rows, (int)len, (long long)src_elems);
    TG_REQUIRE(table_bytes >= (int64_t)n_windows * PP_SLICE_WORDS * 8, "tg_clip_slices: window table of %lld bytes, %lld needed (%d windows of 32 bytes)",
               (long long)table_bytes, (long long)n_windows * PP_SLICE_WORDS * 8, (int)n_windows);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(table) & 7u) == 0 && (reinterpret_cast<uintptr_t>(src) & (unsigned)(elem_bytes - 1)) == 0 &&
               (reinterpret_cast<uintptr_t>(dst) & (unsigned)(elem_bytes - 1)) == 0, "tg_clip_slices: misaligned pointer (table 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    int64_t per = ((int64_t)rows * len + 2047) / 2048;
    per = per < 1 ? 1 : (per > 64 ? 64 : per);
    const dim3 grid((unsigned)n_windows, (unsigned)per);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(pp_slices_kernel<uint16_t>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(src), (long)src_elems, (int)rows,
                           static_cast<const long*>(table), (int)len, static_cast<uint16_t*>(dst));
    else
        hipLaunchKernelGGL(pp_slices_kernel<uint32_t>, grid, dim3(256), 0, s, static_cast<const uint32_t*>(src), (long)src_elems, (int)rows,
                           static_cast<const long*>(table), (int)len, static_cast<uint32_t*>(dst));
    return check_launch("tg_clip_slices");
}

extern "C" int tg_motion_stats_query(int64_t n_rows, int64_t* sizes) {
    TG_REQUIRE(sizes, "tg_motion_stats_query: sizes is NULL");
    TG_REQUIRE(n_rows >= 1 && n_rows < PP_MAX_ROWS, "tg_motion_stats_query: n_rows = %lld must be positive", (long long)n_rows);
    sizes[0] = pp_stats_wgs(n_rows);
    sizes[1] = sizes[0] * PP_ST_COLS * (int64_t)sizeof(double);
    return 0;
}

extern "C" int tg_motion_stats(const void* skel, int64_t n_rows, int32_t half, void* ws, int64_t ws_bytes, void* out, void* stream) {
    TG_REQUIRE(skel && ws && out, "tg_motion_stats: NULL pointer argument");
    TG_REQUIRE(half == 0 || half == 1, "tg_motion_stats: half must be 0 (fp32) or 1 (fp16)");
    TG_REQUIRE(n_rows >= 1 && n_rows < PP_MAX_ROWS, "tg_motion_stats: n_rows = %lld must be positive", (long long)n_rows);
    const int wgs = pp_stats_wgs(n_rows);
    const int64_t need = (int64_t)wgs * PP_ST_COLS * (int64_t)sizeof(double);
    TG_REQUIRE(ws_bytes >= need, "tg_motion_stats: workspace of %lld bytes, %lld needed (tg_motion_stats_query)", (long long)ws_bytes, (long long)need);
    TG_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 &&
               (reinterpret_cast<uintptr_t>(skel) & (half ? 1u : 3u)) == 0, "tg_motion_stats: misaligned pointer (ws / out 8 bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (half)
        hipLaunchKernelGGL(pp_stats_kernel<_Float16>, dim3(wgs), dim3(PP_ST_THREADS), 0, s, static_cast<const _Float16*>(skel), (long)n_rows, static_cast<double*>(ws));
    else
        hipLaunchKernelGGL(pp_stats_kernel<float>, dim3(wgs), dim3(PP_ST_THREADS), 0, s, static_cast<const float*>(skel), (long)n_rows, static_cast<double*>(ws));
    if (check_launch("tg_motion_stats(partials)")) return 1;
    hipLaunchKernelGGL(pp_stats_final_kernel, dim3(1), dim3(PP_ST_THREADS), 0, s, (const double*)static_cast<double*>(ws), wgs, (long)n_rows, static_cast<double*>(out));
    return check_launch("tg_motion_stats(final)");
}
