// tg_tcn_fwd_fused: the text encoder's TCN forward -- four TemporalBlocks of two weight-normed causal convs (kernel 2, dilation 1 / 2 / 4 / 8,
// 300 -> 300 channels; each conv + ReLU + dropout, then relu(out + x)) and the Linear(300, 32) decoder -- as ONE launch.
//
// Everything between the embedding and the GRU input is local to a clip (no BatchNorm, no coupling between clips), so a 512-thread
// workgroup owns R = 2 whole clips (68 rows, five 16-row MFMA tiles) from the embedding output to the 32 decoder columns:
//   * the activation lives in LDS as the fp16 x 2 operand (common.hpp): hi / lo planes of every row scaled by ITS OWN power of two.  It is
//     split once per conv by the epilogue that produced it -- not once per column tile by mover waves, as gemm_mw.hip has to;
//   * the weight operand is the pre-split plane buffer of the eight packed convs ([8 x 300 rows][600] in the slab-tiled layout of
//     common.hpp).  Wave w owns the output-channel tiles w, w + 8, w + 16 of all 68 rows, so every weight fragment is needed by exactly one
//     wave: it goes global (L2) -> registers, one slab ahead, as the MFMA's first operand -- one 16-byte piece per lane, 1 KB of contiguous
//     memory per instruction -- and never through LDS;
//   * the two taps of an output row read source rows t - d and t, which carry different scales: one accumulator set per tap, combined in the
//     epilogue with the two exact inverse scales.  A row much smaller than its neighbours therefore keeps its own relative accuracy.
//     K = [tap 0: 300 | tap 1: 300] puts the tap boundary inside slab 9 (300 = 9 x 32 + 12): that slab is multiplied once per tap, the
//     other tap's 8-byte pieces of the activation fragment pointing at a zero word (2 x 10 slabs instead of 19);
//   * the block input stays in LDS as fp32 for the residual; the epilogues write the taped tensors (o0, o1, y of every block) for the clips
//     of [save_row0, save_row0 + save_rows) only -- nothing else leaves the workgroup except the decoder columns;
//   * the dropout scales are regenerated from the counter RNG (element j * clips * T * C + i of the site, as ops.Drop defines it and the
//     backward's act_mask_bwd kernels regenerate it).
// No synchronisation between workgroups, no global atomics: workgroup barriers only (two per conv), every loop with a static trip count.
// The row maxima are combined across the eight waves by an LDS integer max of non-negative float bit patterns: order-independent, so the
// result is bit-identical from run to run.
//
// LDS: 68 x 300 fp32 block input 81 600 B | 2 planes x 68 x 600 B = 81 600 B | 16 B zero | 2 x 68 row maxima 544 B = 163 760 of 163 840 B.
#include "operand_split.hpp"
#include <stdlib.h>
#include <type_traits>

namespace tg {

constexpr int TF_T = 34, TF_C = 300, TF_R = 2, TF_ROWS = TF_R * TF_T, TF_MT = 5, TF_NTILES = 19, TF_BLOCKS = 4, TF_E = 32;
constexpr int TF_ROWB = TF_C * 2;                       // bytes of one plane row (150 dwords: 16 consecutive rows start in 16 different even banks)
constexpr int TF_PLANE = TF_ROWS * TF_ROWB;
constexpr int TF_X_OFF = 0, TF_PL_OFF = TF_ROWS * TF_C * 4, TF_ZERO_OFF = TF_PL_OFF + 2 * TF_PLANE, TF_RMAX_OFF = TF_ZERO_OFF + 16;
constexpr int TF_LDS = TF_RMAX_OFF + 2 * TF_ROWS * 4;
constexpr int TF_Q_TAP = TF_C / 4;                      // 8-byte pieces (4 channels) per tap
static_assert(TF_LDS <= 163840 && TF_PL_OFF % 16 == 0 && TF_PLANE % 8 == 0 && TF_ROWB % 8 == 0, "LDS layout");

struct TcnArgs {
    const float* x0;                 // [clips][T][C]: the embedding-dropout output
    const unsigned char* wpl;        // fp16 x 2 planes of the packed conv weights, [8 C rows + zero row][2 C] slab-tiled
    long wplane_b;                   // bytes between the hi and the lo plane
    unsigned wslab_b;                // bytes of one 32-column slab of a plane
    int wzero_row;                   // the buffer's all-zero row
    const float* winv;               // inverse scales of the weight rows
    const float* bias[2 * TF_BLOCKS];
    const float* dec_w;              // [32][C]
    const float* dec_b;
    const uint64_t* drop;            // Philox state (nullptr: no dropout)
    unsigned site;
    float p;
    int clips;
    float *o0, *o1, *y;              // taped tensors, [blocks][clips][T][C] each
    int save0, save1;                // taped clips: [save0, save1)
    float* out;                      // decoder columns: row (clip * T + t) at out + row * out_ld
    long out_ld;
};

struct TfW { tg_f16x8 hi, lo; };

// NJ: column tiles of this wave (19 tiles over 8 waves: waves 0-2 own three, the others two).  A compile-time count: a wave-uniform `if`
// around the third tile's matrix instructions cut the K loop into basic blocks the scheduler could not interleave loads and MFMAs across.
template <int NJ>
__device__ __forceinline__ void tcn_fwd_fused_body(const TcnArgs& a, unsigned char* const smem) {
    float* const xres = reinterpret_cast<float*>(smem + TF_X_OFF);
    unsigned char* const pl = smem + TF_PL_OFF;
    unsigned* const rmax = reinterpret_cast<unsigned*>(smem + TF_RMAX_OFF);
    constexpr int ZREL = TF_ZERO_OFF - TF_PL_OFF;          // the zero word, relative to the planes
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int r16 = lane & 15, kq = lane >> 4;
    const int clip0 = blockIdx.x * TF_R;
    const int nclip = a.clips - clip0 < TF_R ? a.clips - clip0 : TF_R;

    auto store_planes = [&](int row, int col, const f32x4 v, float s) __attribute__((always_inline)) {
        unsigned h0, l0, h1, l1;
        h2_split2(v[0] * s, v[1] * s, h0, l0);
        h2_split2(v[2] * s, v[3] * s, h1, l1);
        unsigned char* const q = pl + row * TF_ROWB + col * 2;
        *reinterpret_cast<u32x2*>(q) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(q + TF_PLANE) = u32x2{l0, l1};
    };
    auto absmax4 = [](unsigned m, const f32x4 v) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float f = v[q]; const unsigned b = __float_as_uint(f) & 0x7fffffffu; m = m > b ? m : b; }
        return m;
    };

    // ---- the workgroup's clips -> LDS (a clip past the batch reads as zeros and is never written anywhere), then row by row into the planes
    {
        const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(a.x0 + (long)clip0 * (TF_T * TF_C));
        const int live = nclip * (TF_T * TF_C / 4);
        for (int i = t; i < TF_ROWS * TF_C / 4; i += 512) reinterpret_cast<f32x4*>(xres)[i] = i < live ? src[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < 4) reinterpret_cast<unsigned*>(smem + TF_ZERO_OFF)[t] = 0u;
        if (t < TF_ROWS) rmax[t] = 0u;
    }
    __syncthreads();
    for (int row = wave; row < TF_ROWS; row += 8) {
        const float* xr = xres + row * TF_C;
        const bool two = lane + 64 < TF_C / 4;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(xr + 4 * lane);
        const f32x4 v1 = two ? *reinterpret_cast<const f32x4*>(xr + 4 * (lane + 64)) : f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned mx = wave_max_u32(absmax4(absmax4(0u, v0), v1));
        const float s = h2_scale_of_exp(h2_exp_of_bits(mx));
        if (lane == 0) rmax[TF_ROWS + row] = mx;
        store_planes(row, 4 * lane, v0, s);
        if (two) store_planes(row, 4 * (lane + 64), v1, s);
    }
    __syncthreads();

    // ---- per-lane constants: product rows 16 i + r16, their clip / time step / global row
    int rowoff1[TF_MT];                                    // byte offset of row m inside a plane, -1 past the workgroup's rows
    int tl[TF_MT];
    int goff[TF_MT];                                       // element offset of the row in a [clips][T][C] tensor (clips <= 2^16: below 2^30)
    bool rowok[TF_MT], saved[TF_MT], gok[TF_MT];
#pragma unroll
    for (int i = 0; i < TF_MT; ++i) {
        const int m = 16 * i + r16;
        rowok[i] = m < TF_ROWS;
        const int mm = rowok[i] ? m : 0;
        const int c = mm >= TF_T ? 1 : 0;
        tl[i] = mm - c * TF_T;
        rowoff1[i] = rowok[i] ? m * TF_ROWB : -1;
        gok[i] = rowok[i] && c < nclip;
        const int clip = gok[i] ? clip0 + c : 0;
        saved[i] = gok[i] && clip >= a.save0 && clip < a.save1;
        goff[i] = (clip * TF_T + tl[i]) * TF_C;
    }
    const long per = (long)a.clips * (TF_T * TF_C);        // elements per dropout site
    const bool drop_on = a.drop != nullptr && a.p > 0.f;

    f32x4 acc[2][TF_MT][NJ];

    for (int j = 0; j < 2 * TF_BLOCKS; ++j) {
        const int d = 1 << (j >> 1);
        const bool second = j & 1;
        int rowoff0[TF_MT];                                // the dilated tap: row m - d of the same clip, -1 (zero) for t < d
#pragma unroll
        for (int i = 0; i < TF_MT; ++i) rowoff0[i] = (rowok[i] && tl[i] >= d) ? rowoff1[i] - d * TF_ROWB : -1;
        // weight fragments: row (j C + n) of the plane buffer, n = 16 (wave + 8 jn) + r16; rows past C read the zero row
        unsigned woff[NJ];
#pragma unroll
        for (int jn = 0; jn < NJ; ++jn) {
            const int n = 16 * (wave + 8 * jn) + r16;
            woff[jn] = (unsigned)(n < TF_C ? j * TF_C + n : a.wzero_row) * 64u + (unsigned)kq * 16u;
        }
        auto load_w = [&](int s, TfW (&w)[NJ]) __attribute__((always_inline)) {
            const unsigned char* __restrict__ base = a.wpl + (size_t)s * a.wslab_b;
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) {
                w[jn].hi = *reinterpret_cast<const tg_f16x8*>(base + woff[jn]);
                w[jn].lo = *reinterpret_cast<const tg_f16x8*>(base + a.wplane_b + woff[jn]);
            }
        };
        // one 32-deep slab of tap TAP: the lane's fragment of the activation is two 8-byte pieces (4 channels each; a piece never straddles
        // the tap boundary), each either inside the tap's source row or the zero word
        auto slab = [&](auto tap_c, int s, const TfW (&w)[NJ]) __attribute__((always_inline)) {
            constexpr int TAP = decltype(tap_c)::value;
            int cb[2];
            bool ok[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = 8 * s + 2 * kq + h;
                ok[h] = TAP == 0 ? q < TF_Q_TAP : (q >= TF_Q_TAP && q < 2 * TF_Q_TAP);
                cb[h] = (q - TAP * TF_Q_TAP) * 8;
            }
#pragma unroll
            for (int i = 0; i < TF_MT; ++i) {
                const int ro = TAP ? rowoff1[i] : rowoff0[i];
                u32x2 xh[2], xl[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool v = ok[h] && ro >= 0;
                    xh[h] = *reinterpret_cast<const u32x2*>(pl + (v ? ro + cb[h] : ZREL));
                    xl[h] = *reinterpret_cast<const u32x2*>(pl + (v ? ro + cb[h] + TF_PLANE : ZREL));
                }
                const tg_f16x8 fh = __builtin_bit_cast(tg_f16x8, u32x4{xh[0][0], xh[0][1], xh[1][0], xh[1][1]});
                const tg_f16x8 fl = __builtin_bit_cast(tg_f16x8, u32x4{xl[0][0], xl[0][1], xl[1][0], xl[1][1]});
                // lo_w hi_x + hi_w lo_x + hi_w hi_x (smallest terms first, as gemm_mw.hip)
                // (term-major over the column tiles: the instructions that accumulate into one tile are NJ issues apart)
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) acc[TAP][i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[jn].lo, fh, acc[TAP][i][jn], 0, 0, 0);
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) acc[TAP][i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[jn].hi, fl, acc[TAP][i][jn], 0, 0, 0);
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) acc[TAP][i][jn] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[jn].hi, fh, acc[TAP][i][jn], 0, 0, 0);
            }
        };
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int i = 0; i < TF_MT; ++i)
#pragma unroll
                for (int jn = 0; jn < NJ; ++jn) acc[q][i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};

        using tap0 = std::integral_constant<int, 0>;
        using tap1 = std::integral_constant<int, 1>;
        TfW w0[NJ], w1[NJ];
        load_w(0, w0);
        for (int s = 0; s < 10; s += 2) {                  // tap 0: slabs 0 .. 9
            load_w(s + 1, w1);
            slab(tap0{}, s, w0);
            load_w(s + 2 < 10 ? s + 2 : 9, w0);            // (after slab 8: slab 9 again, the first of tap 1)
            slab(tap0{}, s + 1, w1);
        }
        for (int s = 9; s < 19; s += 2) {                  // tap 1: slabs 9 .. 18
            load_w(s + 1, w1);
            slab(tap1{}, s, w0);
            load_w(s + 2 < 19 ? s + 2 : 18, w0);
            slab(tap1{}, s + 1, w1);
        }

        // ---- epilogue, part A: scale back, bias, ReLU, dropout, (second conv) residual + ReLU; taped stores; row maxima of what the next conv reads
        const unsigned* const rm_in = rmax + ((j + 1) & 1) * TF_ROWS;      // maxima of the rows this conv has read
        unsigned* const rm_out = rmax + (j & 1) * TF_ROWS;                   // ... of the rows it writes (zero since the conv before last)
        const float* __restrict__ bias = a.bias[j];
        const float* __restrict__ winv = a.winv + j * TF_C;
        float* __restrict__ const tape0 = (second ? a.o1 : a.o0) + (long)(j >> 1) * per;
        float* __restrict__ const tape_y = a.y + (long)(j >> 1) * per;
#pragma unroll
        for (int i = 0; i < TF_MT; ++i) {
            const int m = rowok[i] ? 16 * i + r16 : 0;
            const float inv1 = h2_inv_of_exp(h2_exp_of_bits(rm_in[m]));
            const float inv0 = h2_inv_of_exp(h2_exp_of_bits(rm_in[tl[i] >= d ? m - d : m]));
            unsigned mx = 0u;
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) {
                const int n = 16 * (wave + 8 * jn) + 4 * kq;
                const bool cok = n < TF_C;                 // (tile 18 ends at column 300)
                const int nn = cok ? n : 0;
                const f32x4 iw = *reinterpret_cast<const f32x4*>(winv + nn);
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + nn);
                // two exact power-of-two steps per tap: the pair's product could leave fp32's range
                f32x4 v = (acc[0][i][jn] * inv0) * iw + (acc[1][i][jn] * inv1) * iw + bv;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = v[q] > 0.f ? v[q] : 0.f;
                if (drop_on) v *= dropout_scale4(a.drop, a.site, a.p, (unsigned long)(j * per + goff[i] + nn) >> 2);
                if (saved[i] && cok) *reinterpret_cast<f32x4*>(tape0 + goff[i] + nn) = v;
                if (second) {
                    float* const xp = xres + m * TF_C + nn;
                    const f32x4 x = *reinterpret_cast<const f32x4*>(xp);
                    v += x;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = v[q] > 0.f ? v[q] : 0.f;
                    if (rowok[i] && cok) *reinterpret_cast<f32x4*>(xp) = v;
                    if (saved[i] && cok) *reinterpret_cast<f32x4*>(tape_y + goff[i] + nn) = v;
                }
                if (cok) mx = absmax4(mx, v);
                acc[1][i][jn] = v;
            }
            unsigned o = (unsigned)__shfl_xor((int)mx, 16, 64); mx = mx > o ? mx : o;
            o = (unsigned)__shfl_xor((int)mx, 32, 64); mx = mx > o ? mx : o;
            if (kq == 0 && rowok[i]) atomicMax(rm_out + m, mx);
        }
        __syncthreads();
        if (j == 2 * TF_BLOCKS - 1) break;
        // ---- part B: every wave has left the K loop and every row maximum is final: the planes are overwritten with this conv's output
        if (t < TF_ROWS) rmax[((j + 1) & 1) * TF_ROWS + t] = 0u;
#pragma unroll
        for (int i = 0; i < TF_MT; ++i) {
            const int m = rowok[i] ? 16 * i + r16 : 0;
            const float s = h2_scale_of_exp(h2_exp_of_bits(rm_out[m]));
#pragma unroll
            for (int jn = 0; jn < NJ; ++jn) {
                const int n = 16 * (wave + 8 * jn) + 4 * kq;
                if (rowok[i] && n < TF_C) store_planes(m, n, acc[1][i][jn], s);
            }
        }
        __syncthreads();
    }

    // ---- decoder: Linear(C, 32) on the last block's output (fp32 in LDS), plain fp32 FMAs: thread (column c, rows mg + 16 k)
    {
        const int c = t & 31, mg = t >> 5;
        const float* __restrict__ wr = a.dec_w + c * TF_C;
        float s[TF_MT];
        int mrow[TF_MT];
#pragma unroll
        for (int k = 0; k < TF_MT; ++k) { s[k] = 0.f; const int m = mg + 16 * k; mrow[k] = (m < TF_ROWS ? m : 0) * TF_C; }
        for (int k4 = 0; k4 < TF_C; k4 += 4) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(wr + k4);
#pragma unroll
            for (int k = 0; k < TF_MT; ++k) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(xres + mrow[k] + k4);
                s[k] = fmaf(w[0], x[0], s[k]); s[k] = fmaf(w[1], x[1], s[k]); s[k] = fmaf(w[2], x[2], s[k]); s[k] = fmaf(w[3], x[3], s[k]);
            }
        }
        const float b = a.dec_b[c];
#pragma unroll
        for (int k = 0; k < TF_MT; ++k) {
            const int m = mg + 16 * k;
            const int cl = m >= TF_T ? 1 : 0;
            if (m < TF_ROWS && cl < nclip) a.out[((long)(clip0 + cl) * TF_T + (m - cl * TF_T)) * a.out_ld + c] = s[k] + b;
        }
    }
}

__global__ __launch_bounds__(512, 1) void tcn_fwd_fused_kernel(const TcnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[TF_LDS];
    // (both instantiations pass the same barriers in the same order)
    if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) + 16 < TF_NTILES) tcn_fwd_fused_body<3>(a, smem);
    else tcn_fwd_fused_body<2>(a, smem);
}

}  // namespace tg

using namespace tg;

extern "C" int tg_get_math_mode(void);

static bool tcn_fused_envelope(int T, int C, int n_blocks) { return T == TF_T && C == TF_C && n_blocks == TF_BLOCKS && tg_get_math_mode() == 0; }

extern "C" int tg_tcn_fwd_fused(const float* x0, const void* w_planes, int64_t w_plane_stride, int32_t w_rows, const float* w_inv, const float* const* biases,
                                const float* dec_w, const float* dec_b, const uint64_t* rng_state, uint32_t site, float p, int32_t clips, int32_t T,
                                int32_t C, int32_t n_blocks, float* o0, float* o1, float* y, int32_t save_row0, int32_t save_rows, float* out,
                                int64_t out_ld, void* stream) {
    TG_REQUIRE(x0 && w_planes && w_inv && biases && dec_w && dec_b && out, "tg_tcn_fwd_fused: null argument");
    TG_REQUIRE(clips > 0 && clips <= (1 << 16), "tg_tcn_fwd_fused: clips must be in [1, 2^16]");
    TG_REQUIRE(tcn_fused_envelope(T, C, n_blocks), "tg_tcn_fwd_fused: envelope is T = %d, C = %d, %d blocks, fp32-accurate mode", TF_T, TF_C, TF_BLOCKS);
    constexpr int cwp = (2 * TF_C + 31) / 32 * 32;
    TG_REQUIRE(w_rows == 2 * TF_BLOCKS * TF_C && w_plane_stride == (int64_t)(w_rows + 1) * cwp,
               "tg_tcn_fwd_fused: the weight planes must hold %d rows of %d columns (fp16 x 2, slab-tiled)", 2 * TF_BLOCKS * TF_C, 2 * TF_C);
    TG_REQUIRE(p >= 0.f && p < 1.f && (p == 0.f || rng_state), "tg_tcn_fwd_fused: 0 <= p < 1, and a Philox state when p > 0");
    TG_REQUIRE(save_row0 >= 0 && save_rows >= 0 && (int64_t)save_row0 + save_rows <= clips, "tg_tcn_fwd_fused: taped clips outside the batch");
    TG_REQUIRE(save_rows == 0 || (o0 && o1 && y), "tg_tcn_fwd_fused: taped clips need o0 / o1 / y");
    TG_REQUIRE(out_ld >= TF_E, "tg_tcn_fwd_fused: out_ld below the decoder width");
    TG_REQUIRE(aligned16(x0) && aligned16(w_planes) && aligned16(w_inv) && aligned16(dec_w) && aligned16(o0) && aligned16(o1) && aligned16(y),
               "tg_tcn_fwd_fused: 16-byte aligned operands");
    TcnArgs a;
    for (int j = 0; j < 2 * TF_BLOCKS; ++j) {
        TG_REQUIRE(biases[j] && aligned16(biases[j]), "tg_tcn_fwd_fused: bias %d null or misaligned", j);
        a.bias[j] = biases[j];
    }
    a.x0 = x0;
    a.wpl = static_cast<const unsigned char*>(w_planes);
    a.wplane_b = (long)w_plane_stride * 2;
    a.wslab_b = (unsigned)(w_rows + 1) * 64u;
    a.wzero_row = w_rows;
    a.winv = w_inv;
    a.dec_w = dec_w; a.dec_b = dec_b;
    a.drop = p > 0.f ? rng_state : nullptr;
    a.site = site; a.p = p; a.clips = clips;
    a.o0 = o0; a.o1 = o1; a.y = y;
    a.save0 = save_row0; a.save1 = save_row0 + save_rows;
    a.out = out; a.out_ld = out_ld;
    hipLaunchKernelGGL(tcn_fwd_fused_kernel, dim3((clips + TF_R - 1) / TF_R), dim3(512), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("tg_tcn_fwd_fused");
}
