// One time step of a GRU recurrence on the f32 matrix cores: the body that the per-step kernels of gru.hip and gru_seq.hip share.
//
// A workgroup owns [32 batch rows] x [16 hidden units, all three gates]: 8 waves = 2 row tiles x 4 K-slices.  Every wave first issues the
// loads of its gate-epilogue operands (in the kernel) and of ALL its K fragments (16-byte k-permuted MFMA feed, see gemm.hip), then runs its
// MFMAs; partial sums meet in LDS and all eight waves share the fused gate epilogue.  The kernels differ in where a row's clock points, where
// h_prev comes from and what they store; the product and the cell arithmetic below are stated once.
#pragma once
#include "common.hpp"

namespace tg {

constexpr int GRU_MT = 2;   // 16-row tiles per workgroup
constexpr int GRU_KS = 4;   // K slices per workgroup
constexpr int GRU_PF = 5;   // K fragments in flight per wave (covers H <= 320 in one batch of loads)
constexpr int GRU_THREADS = 64 * GRU_MT * GRU_KS;

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return ok ? *reinterpret_cast<const f32x4*>(p) : z;
}

// What a workgroup and a lane own.  brow: the batch row whose A fragments the lane loads.  Gate epilogue ownership: wave (mt, ks) finalises
// accumulator row i = ks of m-tile mt, i.e. element (erow, ej).
struct StepTile {
    int dir, bt, jt, lane, mt, ks, r16, kq, j0, b0, brow, erow, ej;
};

__device__ __forceinline__ StepTile step_tile(int n_jt, int n_bt) {
    StepTile t;
    // logical order: batch tile fastest, then hidden-unit slice, then direction -> an XCD's chunk holds few W_hh slices
    // (57.6 KB each at H = 300) for ALL batch tiles, and one direction's h_{t-1}
    const int lid = xcd_chunked_id(blockIdx.x, gridDim.x);
    t.bt = lid % n_bt; t.jt = (lid / n_bt) % n_jt;
    t.dir = lid / (n_bt * n_jt);
    const int wave = threadIdx.x >> 6;
    t.lane = threadIdx.x & 63;
    t.mt = wave % GRU_MT; t.ks = wave / GRU_MT;
    t.r16 = t.lane & 15; t.kq = t.lane >> 4;
    t.j0 = t.jt * 16; t.b0 = t.bt * (GRU_MT * 16);
    t.brow = t.b0 + t.mt * 16 + t.r16;
    t.erow = t.b0 + t.mt * 16 + t.kq * 4 + t.ks;
    t.ej = t.j0 + t.r16;
    return t;
}

// host side: hidden slices, batch tiles and the grid of one step launch over D directions
struct StepGrid {
    int n_jt, n_bt;
    dim3 grid;
};
inline StepGrid step_grid(int B, int H, int D) {
    const int n_jt = cdiv(H, 16), n_bt = cdiv(B, GRU_MT * 16);
    return {n_jt, n_bt, dim3(n_jt * n_bt * D)};
}

// gh[g] = (h_prev @ W_hh^T)[erow][g * H + ej].  hrow: the lane's h_prev row (read where b_ok); whh: the direction's [3H][H].  `run` is
// launch-uniform: without it nothing is loaded and gh = 0, but every thread still passes the barrier.
__device__ __forceinline__ void step_product_fwd(bool run, const float* hrow, bool b_ok, const float* whh, int H, const StepTile& t,
                                                 float (&red)[GRU_KS][GRU_MT][3][4][64], float (&gh)[3]) {
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (run) {
        const bool j_ok = t.ej < H;
        const float* wrow[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) wrow[g] = whh + (long)(g * H + (j_ok ? t.ej : 0)) * H;
        for (int kbase = t.ks * 16; kbase < H; kbase += GRU_KS * 16 * GRU_PF) {
            f32x4 a[GRU_PF], w[3][GRU_PF];
#pragma unroll
            for (int p = 0; p < GRU_PF; ++p) {
                const int k = kbase + p * (GRU_KS * 16) + 4 * t.kq;
                const bool inb = k < H;   // H % 4 == 0 (checked on the host)
                a[p] = ld4(hrow + k, b_ok && inb);
#pragma unroll
                for (int g = 0; g < 3; ++g) w[g][p] = ld4(wrow[g] + k, j_ok && inb);
            }
#pragma unroll
            for (int p = 0; p < GRU_PF; ++p) {
                if (kbase + p * (GRU_KS * 16) < H) {      // wave-uniform
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][v], w[g][p][v], acc[g], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[t.ks][t.mt][g][i][t.lane] = acc[g][i];
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        float s = red[0][t.mt][g][t.ks][t.lane];
#pragma unroll
        for (int q = 1; q < GRU_KS; ++q) s += red[q][t.mt][g][t.ks][t.lane];
        gh[g] = s;
    }
}

// (dgh_next @ W_hh)[erow][ej].  arow: the lane's dgh row of the consumer step (read where b_ok); wt: the direction's W_hh^T [H][3H].
// `run` as above.
__device__ __forceinline__ float step_product_bwd(bool run, const float* arow, bool b_ok, const float* wt, int H, const StepTile& t,
                                                  float (&red)[GRU_KS][GRU_MT][4][64]) {
    const int H3 = 3 * H;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    if (run) {
        const bool j_ok = t.ej < H;
        const float* wrow = wt + (long)(j_ok ? t.ej : 0) * H3;
        for (int kbase = t.ks * 16; kbase < H3; kbase += GRU_KS * 16 * GRU_PF) {
            f32x4 a[GRU_PF], w[GRU_PF];
#pragma unroll
            for (int p = 0; p < GRU_PF; ++p) {
                const int k = kbase + p * (GRU_KS * 16) + 4 * t.kq;
                const bool inb = k < H3;
                a[p] = ld4(arow + k, b_ok && inb);
                w[p] = ld4(wrow + k, j_ok && inb);
            }
#pragma unroll
            for (int p = 0; p < GRU_PF; ++p) {
                if (kbase + p * (GRU_KS * 16) < H3) {
                    // two accumulators: the dependent-accumulator latency of v_mfma_f32_16x16x4_f32 (40 cycles) exceeds
                    // its issue interval (32)
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][0], w[p][0], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][1], w[p][1], acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][2], w[p][2], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[p][3], w[p][3], acc1, 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) red[t.ks][t.mt][i][t.lane] = acc0[i] + acc1[i];
    __syncthreads();
    float s = red[0][t.mt][t.ks][t.lane];
#pragma unroll
    for (int q = 1; q < GRU_KS; ++q) s += red[q][t.mt][t.ks][t.lane];
    return s;
}

// the cell: hn = W_hn h + b_hn, h = (1 - z) n + z h_prev.  (Which product of h the compiler fuses into an FMA is decided per kernel, after
// inlining: the two files agree within the gates of tests/test_gru_seq_gpu.py, not bit for bit.)
struct GruCell {
    float r, z, n, hn, h;
};
__device__ __forceinline__ GruCell gru_cell_fwd(float gi_r, float gi_z, float gi_n, const float (&gh)[3], float bh_r, float bh_z, float bh_n,
                                                float hp) {
    const float hn = gh[2] + bh_n;
    const float r = gate_sigmoid(gi_r + gh[0] + bh_r);
    const float z = gate_sigmoid(gi_z + gh[1] + bh_z);
    const float n = gate_tanh(gi_n + r * hn);
    const float h = (1.f - z) * n + z * hp;
    return {r, z, n, hn, h};
}

// dn = dh (1-z)(1-n^2),  dz = dh (h_prev - n) z (1-z),  dr = dn * hn * r (1-r)
struct GruCellGrad {
    float dr, dz, dn;
};
__device__ __forceinline__ GruCellGrad gru_cell_bwd(float dh, float r, float z, float n, float hn, float hp) {
    const float dn = dh * (1.f - z) * (1.f - n * n);
    const float dz = dh * (hp - n) * z * (1.f - z);
    const float dr = dn * hn * r * (1.f - r);
    return {dr, dz, dn};
}

// dgi = [dr, dz, dn], dgh = [dr, dz, dn * r] of one element; gi_o / gh_o point at column ej of the position's 3H row
__device__ __forceinline__ void store_gate_grads(float* gi_o, float* gh_o, int H, float dr, float dz, float dn, float dn_r) {
    gi_o[0] = dr; gi_o[H] = dz; gi_o[2 * H] = dn;
    gh_o[0] = dr; gh_o[H] = dz; gh_o[2 * H] = dn_r;
}

}  // namespace tg
