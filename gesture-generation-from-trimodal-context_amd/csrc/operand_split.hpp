// The operand-split layer of the matrix-core kernels: fp32 values -> the packed bf16 / fp16 words the MFMAs read, and the small utilities every
// one of those kernels carries around it.  The arithmetic of one value (split3_bits, pack_hi16, h2_split2, the fp16 x 2 scales) is common.hpp's;
// what is specific to ONE kernel (its LDS stores, per-column scales, exchange-buffer habits) stays in that kernel as a thin wrapper.
#pragma once
#include "common.hpp"
#include <type_traits>
#include <utility>

namespace tg {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), unrolled
template <int N, typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl<N>(f, std::make_integer_sequence<int, N>{}); }

// ---- buffer descriptors ----------------------------------------------------------------------------------------------------------------
constexpr unsigned RSRC3_RAW32 = 0x00020000u;      // descriptor word 3: raw buffer, 32-bit data format, bounds check on the byte offset
constexpr unsigned VOFF_OOB = 0x80000000u;         // voffset of a piece that must read as zero / not be stored (>= num_records: extents are < 2^31)
// a buffer descriptor whose every input is PROVABLY wave-uniform to the compiler (cdna_hip_programming.md T20: otherwise each buffer
// operation is wrapped in a readfirstlane / saveexec "waterfall" loop)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(base);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0, __builtin_amdgcn_readfirstlane(bytes), RSRC3_RAW32);
}

// ---- LDS slab rows ---------------------------------------------------------------------------------------------------------------------
// An LDS row that holds one 32-deep slab row = 64 bytes = four 16-byte slots (slot kq = k 8 kq .. 8 kq + 7), unpadded: the slot index is XORed
// with 2 * bit 3 of the row (gemm_split.hip has the bank arithmetic).  Returned as the XOR for a bf16 COLUMN index.
__device__ __forceinline__ int slab_swz(int row) { return ((row >> 3) & 1) << 4; }

// ---- four / eight consecutive fp32 -> packed operand words -----------------------------------------------------------------------------
// hipcc 7.2: __builtin_bit_cast(unsigned, v[i]) on an ext-vector ELEMENT is miscompiled -- every i reads element 0.  Copy the element to a
// scalar first (`const float x = v[i];`), as every function below does before a value reaches split3_bits.
//
// NS = 1: the plain bf16 tier, rounded to nearest even (v_cvt_pk_bf16_f32).  NS = 3: the exact hi / mid / lo terms of bf16 x 3.
template <int NS>
__device__ __forceinline__ void split4(const f32x4 v, u32x2 (&out)[NS]) {
    if constexpr (NS == 1) {
        typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
        bf16x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (__bf16)v[i];
        out[0] = __builtin_bit_cast(u32x2, r);
    } else {
        static_assert(NS == 3, "1 or 3 terms; fp16 x 2 takes a scale");
        unsigned h[4], m[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x = v[i];
            split3_bits(x, h[i], m[i], l[i]);
        }
        out[0] = u32x2{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3])};
        out[1] = u32x2{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3])};
        out[2] = u32x2{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3])};
    }
}
// fp16 x 2 (common.hpp "two-term fp16 split"): four ALREADY SCALED values -> their hi and lo words
__device__ __forceinline__ void h2_split4(float x0, float x1, float x2, float x3, u32x2 (&out)[2]) {
    unsigned h0, l0, h1, l1;
    h2_split2(x0, x1, h0, l0);
    h2_split2(x2, x3, h1, l1);
    out[0] = u32x2{h0, h1};
    out[1] = u32x2{l0, l1};
}
// ... four values times their power-of-two scale
__device__ __forceinline__ void split4(const f32x4 v, const float scale, u32x2 (&out)[2]) { h2_split4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale, out); }

// eight consecutive fp32 (two float4) -> NS MFMA fragments (fp16 x 2: fp16 bit patterns in bf16x8 registers)
template <int NS>
__device__ __forceinline__ void split8(const f32x4 a, const f32x4 b, bf16x8 (&out)[NS]) {
    if constexpr (NS == 1) {
        bf16x8 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) { r[i] = (__bf16)a[i]; r[4 + i] = (__bf16)b[i]; }
        out[0] = r;
    } else {
        static_assert(NS == 3, "1 or 3 terms; fp16 x 2 takes a scale");
        unsigned h[8], m[8], l[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float xa = a[i], xb = b[i];
            split3_bits(xa, h[i], m[i], l[i]);
            split3_bits(xb, h[4 + i], m[4 + i], l[4 + i]);
        }
        out[0] = __builtin_bit_cast(bf16x8, u32x4{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]), pack_hi16(h[4], h[5]), pack_hi16(h[6], h[7])});
        out[1] = __builtin_bit_cast(bf16x8, u32x4{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]), pack_hi16(m[4], m[5]), pack_hi16(m[6], m[7])});
        out[2] = __builtin_bit_cast(bf16x8, u32x4{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]), pack_hi16(l[4], l[5]), pack_hi16(l[6], l[7])});
    }
}
__device__ __forceinline__ void split8(const f32x4 a, const f32x4 b, const float scale, bf16x8 (&out)[2]) {
    unsigned h[4], l[4];
    h2_split2(a[0] * scale, a[1] * scale, h[0], l[0]);
    h2_split2(a[2] * scale, a[3] * scale, h[1], l[1]);
    h2_split2(b[0] * scale, b[1] * scale, h[2], l[2]);
    h2_split2(b[2] * scale, b[3] * scale, h[3], l[3]);
    out[0] = __builtin_bit_cast(bf16x8, u32x4{h[0], h[1], h[2], h[3]});
    out[1] = __builtin_bit_cast(bf16x8, u32x4{l[0], l[1], l[2], l[3]});
}

// ---- plane buffers (layout: common.hpp plane_tiled_off; kernels: planes.hip, elementwise.hip) -------------------------------------------------
// one 8-column piece of such a buffer: columns c .. c + 7 (c % 8 == 0) of row r of the fp32 matrix (row stride ldx)
__device__ __forceinline__ void split3_write_piece(const float* __restrict__ x, long ldx, int rows, int cw, int cwp, __bf16* __restrict__ planes,
                                                   long plane_stride, long r, int c, bool vec) {
    float v[8];
    if (r < rows && vec && c + 8 <= cw) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * ldx + c), b = *reinterpret_cast<const f32x4*>(x + r * ldx + c + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (r < rows && c + q < cw) ? x[r * ldx + c + q] : 0.f;
    }
    unsigned h[8], m[8], l[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) split3_bits(v[q], h[q], m[q], l[q]);
    const long o = plane_tiled_off(r, c, rows);
    *reinterpret_cast<u32x4*>(planes + o) = u32x4{pack_hi16(h[0], h[1]), pack_hi16(h[2], h[3]), pack_hi16(h[4], h[5]), pack_hi16(h[6], h[7])};
    *reinterpret_cast<u32x4*>(planes + plane_stride + o) = u32x4{pack_hi16(m[0], m[1]), pack_hi16(m[2], m[3]), pack_hi16(m[4], m[5]), pack_hi16(m[6], m[7])};
    *reinterpret_cast<u32x4*>(planes + 2 * plane_stride + o) = u32x4{pack_hi16(l[0], l[1]), pack_hi16(l[2], l[3]), pack_hi16(l[4], l[5]), pack_hi16(l[6], l[7])};
}

// One WAVE writes row r (r <= rows; r == rows is the all-zero row) of the fp16 x 2 plane buffer of an fp32 matrix [rows][cw] (row stride ldx):
// two fp16 planes (hi / lo of x * s_r) in the slab-tiled layout of plane_tiled_off, `plane_stride` elements apart, and inv[r] = 1 / s_r.
__device__ __forceinline__ void h2_write_row(const float* __restrict__ x, long ldx, int rows, int cw, int cwp, _Float16* __restrict__ planes,
                                             long plane_stride, float* __restrict__ inv, long r, int lane, bool vec) {
    const int c8n = cwp / 8;
    const bool live = r < rows;
    unsigned mx = 0;
    if (live) {
        for (int c = lane * 4; c < cw; c += 256) {
            if (vec && c + 4 <= cw) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
#pragma unroll
                for (int q = 0; q < 4; ++q) { const float f = v[q]; const unsigned b = __float_as_uint(f) & 0x7fffffffu; mx = mx > b ? mx : b; }
            } else {
                for (int q = 0; q < 4 && c + q < cw; ++q) { const unsigned b = __float_as_uint(x[r * ldx + c + q]) & 0x7fffffffu; mx = mx > b ? mx : b; }
            }
        }
        mx = wave_max_u32(mx);
    }
    const int e = h2_exp_of_bits(mx);
    const float s = h2_scale_of_exp(e);
    if (lane == 0) inv[r] = live ? h2_inv_of_exp(e) : 0.f;
    for (int p8 = lane; p8 < c8n; p8 += 64) {
        const int c = p8 * 8;
        float v[8];
        if (live && vec && c + 8 <= cw) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(x + r * ldx + c), b = *reinterpret_cast<const f32x4*>(x + r * ldx + c + 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] = a[q]; v[4 + q] = b[q]; }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = (live && c + q < cw) ? x[r * ldx + c + q] : 0.f;
        }
        unsigned h[4], l[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) h2_split2(v[2 * q] * s, v[2 * q + 1] * s, h[q], l[q]);
        const long o = plane_tiled_off(r, c, rows);
        *reinterpret_cast<u32x4*>(planes + o) = u32x4{h[0], h[1], h[2], h[3]};
        *reinterpret_cast<u32x4*>(planes + plane_stride + o) = u32x4{l[0], l[1], l[2], l[3]};
    }
}

// fp16 x 2 planes of the K-CONCATENATED TRANSPOSE of two matrices: out row n (n < cols), column k (k < 2 rows) = w{k / rows}[k % rows][n], w0 / w1
// [rows][cols] fp32 contiguous -- the weight operand of dx = [dgi_fwd | dgi_rev] @ [W_ih_fwd ; W_ih_rev] (one product over K = 6H) straight from
// the two nn.GRU parameters.  One 256-thread workgroup per 8 output rows: thread (n_l = t % 8, kg = t / 8): a read instruction fetches 32-byte
// pieces of eight source rows, and a thread walks only 2 rows / 32 columns per pass (round 6, first form: 32 rows per workgroup -- 19 workgroups
// per matrix, 225 dependent-latency loads per thread: 100 us for three layers).  `wg` of `nwg` workgroups walk the row blocks; planes as
// h2_write_row writes them (zero row `cols` included).
constexpr int H2_TCAT_ROWS = 8;
__device__ __forceinline__ void h2_planes_tcat_block(const float* __restrict__ w0, const float* __restrict__ w1, int rows, int cols, int cwp,
                                                     _Float16* __restrict__ planes, long plane_stride, float* __restrict__ inv, int wg, int nwg,
                                                     unsigned (&smax)[32][H2_TCAT_ROWS]) {
    const int t = threadIdx.x, n_l = t & 7, kg = t >> 3;
    const int K = 2 * rows;
    for (int n0 = wg * H2_TCAT_ROWS; n0 <= cols; n0 += nwg * H2_TCAT_ROWS) {
        const int n = n0 + n_l;
        const bool live = n < cols;
        unsigned mx = 0u;
        if (live)
            for (int k = kg; k < K; k += 32) {
                const float v = (k < rows ? w0 : w1)[(long)(k < rows ? k : k - rows) * cols + n];
                const unsigned b = __float_as_uint(v) & 0x7fffffffu;
                mx = mx > b ? mx : b;
            }
        smax[kg][n_l] = mx;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 32; ++q) { const unsigned b = smax[q][n_l]; mx = mx > b ? mx : b; }
        __syncthreads();
        const int e = h2_exp_of_bits(mx);
        const float sc = h2_scale_of_exp(e);
        if (kg == 0 && n <= cols) inv[n] = live ? h2_inv_of_exp(e) : 0.f;
        if (n <= cols)
            for (int p8 = kg; p8 < cwp / 8; p8 += 32) {
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int k = 8 * p8 + q;
                    v[q] = (live && k < K) ? (k < rows ? w0 : w1)[(long)(k < rows ? k : k - rows) * cols + n] : 0.f;
                }
                unsigned h[4], l[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) h2_split2(v[2 * q] * sc, v[2 * q + 1] * sc, h[q], l[q]);
                const long o = plane_tiled_off(n, 8 * p8, cols);
                *reinterpret_cast<u32x4*>(planes + o) = u32x4{h[0], h[1], h[2], h[3]};
                *reinterpret_cast<u32x4*>(planes + plane_stride + o) = u32x4{l[0], l[1], l[2], l[3]};
            }
    }
}

}  // namespace tg
