// Long-utterance synthesis on the device: what scripts/synthesize.py:generate_gestures does on the host around every window forward.
//   tg_window_stage      window i's inputs of B utterances in lock-step (:82-119): the audio slice followed by zeros, and the per-frame word
//                        ids (or seq2seq's [SOS, words ..., EOS] list) copied from the utterance's plan.  The plan (synthesize.utterance_plan)
//                        holds integers only -- every floating-point decision (slice start, frame of a word) was taken by the host's Python
//                        doubles once per utterance -- so the result is bit for bit what synthesize.window_inputs returns.  Each row's window
//                        index comes from device memory: the launch is the same for every window.
//   tg_spec_stage        the speech2gesture sibling (:86-93): the (n_mels, width) slice of the utterance's log-mel spectrogram, zeros past its end.
//   tg_utterance_finish  on the stacked windows total [B][F][D]: (a) seq2seq's cubic least-squares smoothing around every window start
//                        (:162-185), (b) the fade-out to the mean pose (:188-207: zero from end_frame - n_pre, weighted quadratic fit over
//                        2 n_pre frames), (c) joint positions of dir_vec + mean_dir_vec (utils/data_utils.py:77-98) in fp64.  A least-squares
//                        fit on the fixed abscissae 0 .. n-1 is a projection y -> P y: the host builds the n x n matrices from n_pre in fp64,
//                        the kernels accumulate P y in fp64 and round once to fp32, as numpy does when it assigns into the fp32 array.
// Plain loads and stores; no workgroup depends on another.  Compiled with -ffp-contract=off (multiply, then add, like numpy's doubles).
#include "window_rows.hpp"

namespace tg {

constexpr int UT_PLAN_COLS = 4;        // plan_win row: audio_start, n_valid, spec_start, text length
constexpr int UT_MAX_PRE = PL_MAX_PRE; // (the fits' tables: window_rows.hpp)

// window of row b: its scheduled index clamped to the utterance's own windows (a finished utterance idles on its last one)
__device__ __forceinline__ long plan_row(const int32_t* __restrict__ win_off, const int32_t* __restrict__ win_idx, int b) {
    const int w0 = win_off[b], nw = win_off[b + 1] - w0;
    int j = win_idx[b];
    j = j < 0 ? 0 : (j >= nw ? nw - 1 : j);
    return (long)w0 + j;
}

__global__ __launch_bounds__(256) void window_stage_kernel(const float* __restrict__ audio, const int64_t* __restrict__ audio_off,
                                                           const int32_t* __restrict__ win_off, const int32_t* __restrict__ win_idx,
                                                           const int64_t* __restrict__ plan_win, const int64_t* __restrict__ plan_text,
                                                           int text_stride, int L, int text_w, float* __restrict__ out_audio,
                                                           int64_t* __restrict__ out_text) {
    const int b = blockIdx.x;
    const long g = plan_row(win_off, win_idx, b);
    if (out_text && blockIdx.y == 0)
        for (int t = threadIdx.x; t < text_w; t += 256) out_text[(long)b * text_w + t] = plan_text[g * text_stride + t];
    if (!out_audio) return;
    // (window_rows.hpp: the row body, shared with the synthesis queue's staging)
    stage_audio_row(audio + audio_off[b], audio_off[b + 1] - audio_off[b], plan_win[g * UT_PLAN_COLS + 0], plan_win[g * UT_PLAN_COLS + 1],
                    out_audio + (long)b * L, L);
}

// E: the spectrogram's element as an integer of its width (fp16 -- the reference's cast -- or fp32): a copy moves bits
template <typename E>
__global__ __launch_bounds__(128) void spec_stage_kernel(const E* __restrict__ spec, const int64_t* __restrict__ spec_off,
                                                         const int32_t* __restrict__ win_off, const int32_t* __restrict__ win_idx,
                                                         const int64_t* __restrict__ plan_win, int n_mels, int width, E* __restrict__ out) {
    const int b = blockIdx.x, m = blockIdx.y;
    const long g = plan_row(win_off, win_idx, b);
    const long nfr = (spec_off[b + 1] - spec_off[b]) / n_mels;
    long s = plan_win[g * UT_PLAN_COLS + 2];
    s = s < 0 ? 0 : s;
    const E* __restrict__ src = spec + spec_off[b] + (long)m * nfr;
    E* __restrict__ dst = out + ((long)b * n_mels + m) * width;
    for (int t = threadIdx.x; t < width; t += 128) dst[t] = s + t < nfr ? src[s + t] : (E)0;
}

// (a) one thread per (row, window, dimension): frames [i stride, i stride + 3 n_pre) (window 0 too: the reference's start_frame is 0 there, not below)
__global__ __launch_bounds__(64) void utterance_smooth_kernel(float* __restrict__ total, long F, int D, const int32_t* __restrict__ n_win,
                                                              int stride, int n_pre, const double* __restrict__ proj) {
    const int b = blockIdx.x, i = blockIdx.y, d = threadIdx.x;
    if (d >= D || i >= n_win[b]) return;
    project_segment(total + ((long)b * F + (long)i * stride) * D + d, D, 3 * n_pre, proj);     // (window_rows.hpp: shared with the pool's hand-over)
}

// (b) one thread per (row, dimension)
__global__ __launch_bounds__(64) void utterance_fade_kernel(float* __restrict__ total, long F, int D, const int32_t* __restrict__ n_win,
                                                            int stride, int n_pre, const double* __restrict__ proj,
                                                            const int32_t* __restrict__ fade_start) {
    const int b = blockIdx.x, d = threadIdx.x;
    const long start = fade_start[b];
    const int n = 2 * n_pre;
    if (d >= D || start < 0 || start + n > F) return;                // (start <= the row's length <= F - 2 n_pre by the host's checks)
    const long len = (long)n_win[b] * stride + n_pre;
    const long keep = min(len, start + n_pre);                       // frames from here on are zero before the fit: padding, or zeroed
    const double* __restrict__ P = proj + 9 * n_pre * n_pre;         // behind the (3 n_pre)^2 cubic table
    float* __restrict__ row = total + (long)b * F * D + d;
    double v[2 * UT_MAX_PRE];
    for (int k = 0; k < n; ++k) v[k] = start + k < keep ? (double)row[(start + k) * D] : 0.0;
    for (int r = 0; r < n; ++r) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) acc += P[r * n + k] * v[k];
        row[(start + r) * D] = (float)acc;
    }
    for (long f = start + n; f < F; ++f) row[f * D] = 0.f;
}

// the nine bones of utils/data_utils.py:dir_vec_pairs (parent, child, length); joint 0 is the origin
__device__ const int UT_BONE_A[9] = {0, 1, 2, 1, 4, 5, 1, 7, 8};
__device__ const int UT_BONE_B[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
__device__ const double UT_BONE_LEN[9] = {0.26, 0.18, 0.14, 0.22, 0.36, 0.33, 0.22, 0.36, 0.33};

// (c) one thread per (row, frame): joints [B][Fj][10][3] fp64
__global__ __launch_bounds__(64) void utterance_joints_kernel(const float* __restrict__ total, long F, const double* __restrict__ mean,
                                                              double* __restrict__ joints, long Fj) {
    const int b = blockIdx.y;
    const long f = (long)blockIdx.x * 64 + threadIdx.x;
    if (f >= Fj) return;
    const float* __restrict__ v = total + ((long)b * F + f) * 27;
    double pos[10][3] = {};
    for (int j = 0; j < 9; ++j)
        for (int c = 0; c < 3; ++c) pos[UT_BONE_B[j]][c] = pos[UT_BONE_A[j]][c] + UT_BONE_LEN[j] * ((double)v[3 * j + c] + mean[3 * j + c]);
    double* __restrict__ o = joints + ((long)b * Fj + f) * 30;
    for (int j = 0; j < 10; ++j)
        for (int c = 0; c < 3; ++c) o[3 * j + c] = pos[j][c];
}

}  // namespace tg

using namespace tg;

extern "C" int tg_window_stage(const float* audio, const int64_t* audio_off, const int32_t* win_off, const int32_t* win_idx, const int64_t* plan_win,
                               const int64_t* plan_text, int32_t text_stride, int32_t B, int32_t L, int32_t text_w, float* out_audio,
                               int64_t* out_text, void* stream) {
    TG_REQUIRE(win_off && win_idx && plan_win && (out_audio || out_text), "tg_window_stage: null pointer");
    TG_REQUIRE(B > 0 && B <= 65535, "tg_window_stage: bad batch B=%d", B);
    TG_REQUIRE(!out_audio || (audio && audio_off && L > 0), "tg_window_stage: audio output without audio, offsets or a length (L=%d)", L);
    TG_REQUIRE(!out_text || (plan_text && text_w > 0 && text_stride >= text_w), "tg_window_stage: text output needs its table and 0 < text_w <= text_stride (%d, %d)",
               text_w, text_stride);
    hipLaunchKernelGGL(window_stage_kernel, dim3(B, out_audio ? cdiv(L, 1024) + 1 : 1), dim3(256), 0, (hipStream_t)stream, audio, audio_off, win_off,
                       win_idx, plan_win, plan_text, text_stride, L, text_w, out_audio, out_text);
    return check_launch("tg_window_stage");
}

extern "C" int tg_spec_stage(const void* spec, const int64_t* spec_off, const int32_t* win_off, const int32_t* win_idx, const int64_t* plan_win,
                             int32_t B, int32_t n_mels, int32_t width, int32_t elem_bytes, void* out, void* stream) {
    TG_REQUIRE(spec && spec_off && win_off && win_idx && plan_win && out, "tg_spec_stage: null pointer");
    TG_REQUIRE(B > 0 && B <= 65535 && n_mels > 0 && n_mels <= 65535 && width > 0, "tg_spec_stage: bad sizes B=%d n_mels=%d width=%d", B, n_mels, width);
    TG_REQUIRE(elem_bytes == 2 || elem_bytes == 4, "tg_spec_stage: elements of %d bytes (fp16: 2, fp32: 4)", elem_bytes);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(spec_stage_kernel<uint16_t>, dim3(B, n_mels), dim3(128), 0, (hipStream_t)stream, (const uint16_t*)spec, spec_off, win_off,
                           win_idx, plan_win, n_mels, width, (uint16_t*)out);
    else
        hipLaunchKernelGGL(spec_stage_kernel<uint32_t>, dim3(B, n_mels), dim3(128), 0, (hipStream_t)stream, (const uint32_t*)spec, spec_off, win_off,
                           win_idx, plan_win, n_mels, width, (uint32_t*)out);
    return check_launch("tg_spec_stage");
}

extern "C" int tg_utterance_finish(float* total, int64_t F, int32_t B, int32_t D, const int32_t* n_win, int32_t max_win, int32_t n_poses,
                                   int32_t n_pre, int32_t smooth, const double* proj, const int32_t* fade_start, const double* mean, double* joints,
                                   int64_t joints_frames, void* stream) {
    TG_REQUIRE(total && n_win, "tg_utterance_finish: null pointer");
    TG_REQUIRE(B > 0 && B <= 65535 && D > 0 && max_win > 0 && max_win <= 65535 && n_poses > 0 && F > 0, "tg_utterance_finish: bad sizes B=%d D=%d max_win=%d n_poses=%d F=%lld",
               B, D, max_win, n_poses, (long long)F);
    TG_REQUIRE(n_pre >= 1 && n_pre <= UT_MAX_PRE && D <= 64 && n_poses - n_pre >= 3 * n_pre,
               "tg_utterance_finish: outside the envelope 1 <= n_pre <= 8, D <= 64, n_poses - n_pre >= 3 n_pre (n_pre=%d D=%d n_poses=%d)", n_pre, D, n_poses);
    const int stride = n_poses - n_pre;
    const int64_t need = (int64_t)max_win * stride + n_pre + (fade_start ? 2 * n_pre : 0);
    TG_REQUIRE(F >= need, "tg_utterance_finish: rows of %lld frames, %lld needed (max_win * stride + n_pre%s)", (long long)F, (long long)need,
               fade_start ? " + 2 n_pre for the fade-out" : "");
    TG_REQUIRE(!(smooth || fade_start) || proj, "tg_utterance_finish: smoothing / fade-out without the projection tables");
    TG_REQUIRE(!joints || (mean && D == 27 && joints_frames > 0 && joints_frames <= F),
               "tg_utterance_finish: joints need mean_dir_vec, D = 27 and 0 < joints_frames <= F (D=%d joints_frames=%lld)", D, (long long)joints_frames);
    TG_REQUIRE(smooth || fade_start || joints, "tg_utterance_finish: nothing to do");
    hipStream_t s = (hipStream_t)stream;
    if (smooth) {
        hipLaunchKernelGGL(utterance_smooth_kernel, dim3(B, max_win), dim3(64), 0, s, total, (long)F, D, n_win, stride, n_pre, proj);
        if (int rc = check_launch("tg_utterance_finish (smooth)")) return rc;
    }
    if (fade_start) {
        hipLaunchKernelGGL(utterance_fade_kernel, dim3(B), dim3(64), 0, s, total, (long)F, D, n_win, stride, n_pre, proj, fade_start);
        if (int rc = check_launch("tg_utterance_finish (fade-out)")) return rc;
    }
    if (joints) {
        hipLaunchKernelGGL(utterance_joints_kernel, dim3(cdiv(joints_frames, 64), B), dim3(64), 0, s, total, (long)F, mean, joints, (long)joints_frames);
        if (int rc = check_launch("tg_utterance_finish (joints)")) return rc;
    }
    return 0;
}
