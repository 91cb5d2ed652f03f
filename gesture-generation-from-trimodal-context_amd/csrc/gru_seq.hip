// General GRU recurrence (nn.GRU semantics, one layer): one or two directions, per-row lengths, an initial state and the final state.
//
// The primitive behind pack_padded_sequence -> nn.GRU -> pad_packed_sequence (the Seq2Seq text encoder) and behind a GRU that starts from a
// given hidden state (a decoder step, the joint-embedding context encoder).  Structure: ONE LAUNCH PER TIME STEP, the per-step kernels of
// gru.hip with a per-row clock.  No workgroup ever waits on another one: the launch boundary is the only dependency between steps.
//
//  * Step s of the forward handles, for batch row b of length len_b, position t = s (forward direction) or t = len_b - 1 - s (reverse
//    direction, which therefore STARTS at the row's last valid position).  Rows with s >= len_b are idle in the product (their A rows are
//    zero) and write the exact zero of the padded position t = s instead -- y, and the tape, come out fully written without a fill pass.
//  * The recurrent product runs on v_mfma_f32_16x16x4_f32 (true fp32 operands and accumulators); workgroup tiling, product and cell: gru_step.hpp.
//  * Tape [D][B][T][5H]: r, z, n, W_hn h + b_hn, h_prev.  h_prev (the state the step started from: h0 at a row's first step) is taped so
//    that the backward and the W_hh weight gradient (dgh^T @ h_prev) need neither y, h0 nor the row's length to find it.
//  * The backward runs the steps in the opposite order on the same per-row clock (step s handles forward step k = len_b - 1 - s); one extra
//    step (k = -1) forms dh0 when it is asked for.  dgi / dgh are written as exact zeros at t >= len_b.
//  * lengths outside [1, T]: the row is skipped (y = 0, h_n = h0, dgi = dgh = 0, dh0 = dh_n) and the caller's flag word is set; nothing is
//    read or written outside the row's own [T] positions.
#include "gru_step.hpp"    // the workgroup tiling, the product and the cell (shared with gru.hip)

namespace tg {

// effective length of row b: len_b, or 0 (the row is skipped) when the table entry is outside [1, T]
__device__ __forceinline__ int gs_len(const long long* __restrict__ lengths, int b, int T) {
    if (!lengths) return T;
    const long long L = lengths[b];
    return (L < 1 || L > T) ? 0 : (int)L;
}

__global__ __launch_bounds__(GRU_THREADS) void gru_seq_fwd_step_kernel(
    const float* __restrict__ gi, long gi_ds, const float* __restrict__ whh0, const float* __restrict__ whh1,
    const float* __restrict__ bhh0, const float* __restrict__ bhh1, const float* __restrict__ h0, const long long* __restrict__ lengths,
    float* __restrict__ Y, float* __restrict__ hn_out, float* __restrict__ save, long save_ds, int* __restrict__ flag,
    int B, int T, int H, int D, int step, int n_jt, int n_bt) {
    __shared__ float red[GRU_KS][GRU_MT][3][4][64];
    const StepTile t = step_tile(n_jt, n_bt);
    const int dir = t.dir, erow = t.erow, ej = t.ej;
    const float* bhh = dir ? bhh1 : bhh0;
    const long DH = (long)D * H;

    // the gate epilogue's operands go out first
    const bool e_ok = erow < B && ej < H;
    const int eL = erow < B ? gs_len(lengths, erow, T) : 0;
    const bool act = e_ok && step < eL;
    const int tau = dir ? eL - 1 - step : step;
    const int tau_prev = dir ? tau + 1 : tau - 1;
    float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f, hp = 0.f, bh_r = 0.f, bh_z = 0.f, bh_n = 0.f;
    if (act) {
        const float* gip = gi + dir * gi_ds + ((long)erow * T + tau) * (3 * H);
        gi_r = gip[ej]; gi_z = gip[H + ej]; gi_n = gip[2 * H + ej];
        bh_r = bhh[ej]; bh_z = bhh[H + ej]; bh_n = bhh[2 * H + ej];
        if (step > 0) hp = Y[((long)erow * T + tau_prev) * DH + dir * H + ej];
        else if (h0) hp = h0[((long)dir * B + erow) * H + ej];
    }

    const int b = t.brow;
    const int bL = b < B ? gs_len(lengths, b, T) : 0;
    const bool b_ok = step < bL;          // idle and skipped rows feed zeros
    const int bprev = dir ? bL - step : step - 1;           // the position the row's previous step wrote (step > 0)
    const float* hrow = !b_ok ? Y : (step > 0 ? Y + ((long)b * T + bprev) * DH + dir * H : h0 + ((long)dir * B + b) * H);
    float gh[3];
    // (launch-uniform: the first step of a zero initial state has no product)
    step_product_fwd(step > 0 || h0, hrow, b_ok, dir ? whh1 : whh0, H, t, red, gh);
    if (!e_ok) return;
    if (!act) {
        // step >= len: position t = step of this row is padding -- exact zeros in y and in the tape
        Y[((long)erow * T + step) * DH + dir * H + ej] = 0.f;
        if (save) {
            float* sp = save + dir * save_ds + ((long)erow * T + step) * (5 * H);
            sp[ej] = 0.f; sp[H + ej] = 0.f; sp[2 * H + ej] = 0.f; sp[3 * H + ej] = 0.f; sp[4 * H + ej] = 0.f;
        }
        if (step == 0) {                  // (only a skipped row is idle at step 0)
            hn_out[((long)dir * B + erow) * H + ej] = h0 ? h0[((long)dir * B + erow) * H + ej] : 0.f;
            if (flag && dir == 0 && ej == 0) *flag = 1;     // eL == 0: the table entry was outside [1, T]
        }
        return;
    }
    const GruCell c = gru_cell_fwd(gi_r, gi_z, gi_n, gh, bh_r, bh_z, bh_n, hp);
    Y[((long)erow * T + tau) * DH + dir * H + ej] = c.h;
    if (step == eL - 1) hn_out[((long)dir * B + erow) * H + ej] = c.h;
    if (save) {
        float* sp = save + dir * save_ds + ((long)erow * T + tau) * (5 * H);
        sp[ej] = c.r; sp[H + ej] = c.z; sp[2 * H + ej] = c.n; sp[3 * H + ej] = c.hn; sp[4 * H + ej] = hp;
    }
}

// Backward step s: forward step k = len_b - 1 - s of every row, i.e. position tau = len_b - 1 - s (forward direction) or s (reverse).  With
// the gate gradients dgh of the step that consumed h_tau (k + 1, written by the previous launch, at position tau_next):
//     dh_tau = dy_tau + dh_next * z_next + dgh_next @ W_hh        (W_hh passed transposed: [H][3H]);   at s = 0: dy_tau + dh_n
//     dgi = [dr, dz, dn],  dgh = [dr, dz, dn * r]                 (gru_cell_bwd)
// k = -1 (s = len_b; launched only when dh0 is asked for): dh0 = dh_next * z_next + dgh_next @ W_hh of the row's first step.
// s >= len_b: exact zeros into dgi / dgh at the padded position t = s.
__global__ __launch_bounds__(GRU_THREADS) void gru_seq_bwd_step_kernel(
    const float* __restrict__ dY, const float* __restrict__ dhn, const float* __restrict__ save, long save_ds,
    const float* __restrict__ wt0, const float* __restrict__ wt1, const long long* __restrict__ lengths, float* __restrict__ dgi,
    float* __restrict__ dgh, long dg_ds, float* __restrict__ dhbuf, float* __restrict__ dh0, int B, int T, int H, int D, int step,
    int n_jt, int n_bt) {
    __shared__ float red[GRU_KS][GRU_MT][4][64];
    const StepTile t = step_tile(n_jt, n_bt);
    const int dir = t.dir, erow = t.erow, ej = t.ej;
    const int H3 = 3 * H;
    const long DH = (long)D * H;
    const bool has_next = step > 0;       // (launch-uniform; a row with step <= len_b then has a consumer step)

    const bool e_ok = erow < B && ej < H;
    const int eL = erow < B ? gs_len(lengths, erow, T) : 0;
    const bool act = e_ok && step < eL;
    const bool first = e_ok && step == eL;                  // k = -1: the gradient of the initial state
    const int tau = dir ? step : eL - 1 - step;
    const int tau_next = dir ? step - 1 : eL - step;
    float dy = 0.f, r = 0.f, z = 0.f, n = 0.f, hn = 0.f, hp = 0.f, z_next = 0.f, dh_next = 0.f;
    float* dh_w = dhbuf + ((long)(step & 1) * D + dir) * (long)B * H;
    const float* dh_r = dhbuf + ((long)((step & 1) ^ 1) * D + dir) * (long)B * H;
    if (act) {
        dy = dY[((long)erow * T + tau) * DH + dir * H + ej];
        const float* sp = save + dir * save_ds + ((long)erow * T + tau) * (5 * H);
        r = sp[ej]; z = sp[H + ej]; n = sp[2 * H + ej]; hn = sp[3 * H + ej]; hp = sp[4 * H + ej];
    }
    if (act || first) {
        if (has_next) {
            z_next = save[dir * save_ds + ((long)erow * T + tau_next) * (5 * H) + H + ej];
            dh_next = dh_r[(long)erow * H + ej];
        } else if (dhn) {
            dh_next = dhn[((long)dir * B + erow) * H + ej];     // the gradient of h_n enters where the forward left off
            z_next = 1.f;
        }
    }

    const int b = t.brow;
    const int bL = b < B ? gs_len(lengths, b, T) : 0;
    const bool b_ok = step <= bL;         // rows past their first step (and skipped rows: bL = 0 < step) feed zeros
    const int bnext = dir ? step - 1 : bL - step;
    const float* arow = dgh + dir * dg_ds + ((long)(b_ok ? b : 0) * T + (b_ok ? bnext : 0)) * H3;
    const float s = step_product_bwd(has_next, arow, b_ok, dir ? wt1 : wt0, H, t, red);
    if (!e_ok) return;
    float carry;                          // what flows into h_tau from the step that consumed it (or from dh_n)
    {
        // the product is rounded before the sum joins it (no FMA): the value this kernel has always formed, stated so that it does not
        // depend on whether the compiler sees the two in one basic block
#pragma clang fp contract(off)
        carry = dh_next * z_next;
        if (has_next) carry += s;
    }
    const long pos = dir * dg_ds + ((long)erow * T + (act ? tau : step)) * H3 + ej;    // an idle row: t = step is padding
    if (!act) {
        if (first && dh0) dh0[((long)dir * B + erow) * H + ej] = carry;
        if (step < T) store_gate_grads(dgi + pos, dgh + pos, H, 0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float dh = dy + carry;
    const GruCellGrad g = gru_cell_bwd(dh, r, z, n, hn, hp);
    store_gate_grads(dgi + pos, dgh + pos, H, g.dr, g.dz, g.dn, g.dn * r);
    dh_w[(long)erow * H + ej] = dh;
}

inline bool gru_seq_in_envelope(int64_t B, int64_t T, int64_t H, int64_t D) {
    if (!(D == 1 || D == 2) || B < 1 || T < 1 || H < 8 || H > 320 || H % 4 != 0) return false;
    // one workgroup per [32 rows] x [16 units] x direction: the count must fit the launch's int
    return ((B + 31) / 32) * ((H + 15) / 16) * D <= 0x7fffffffLL;
}

}  // namespace tg

using namespace tg;

#define GS_ENVELOPE "D in {1, 2}, B >= 1, T >= 1, H %% 4 == 0, 8 <= H <= 320"

extern "C" int tg_gru_seq_supported(int32_t B, int32_t T, int32_t H, int32_t D, int32_t* supported) {
    TG_REQUIRE(supported, "tg_gru_seq_supported: null pointer");
    TG_REQUIRE(B > 0 && T > 0 && H > 0 && D > 0, "tg_gru_seq_supported: sizes must be positive (B=%d T=%d H=%d D=%d)", B, T, H, D);
    *supported = gru_seq_in_envelope(B, T, H, D) ? 1 : 0;
    return 0;
}

extern "C" int tg_gru_seq_forward(const float* gi, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev,
                                  const float* h0, const void* lengths, float* y, float* h_n, float* save, int32_t* flag, int32_t B, int32_t T,
                                  int32_t H, int32_t D, void* stream) {
    TG_REQUIRE(gru_seq_in_envelope(B, T, H, D), "tg_gru_seq_forward: outside the envelope " GS_ENVELOPE " (B=%d T=%d H=%d D=%d)", B, T, H, D);
    TG_REQUIRE(gi && w_hh_fwd && b_hh_fwd && y && h_n && (D == 1 || (w_hh_rev && b_hh_rev)), "tg_gru_seq_forward: null pointer");
    TG_REQUIRE(aligned16(w_hh_fwd) && aligned16(w_hh_rev) && aligned16(y) && aligned16(h0), "tg_gru_seq_forward: w_hh / y / h0 must be 16-byte aligned");
    TG_REQUIRE(!lengths || (reinterpret_cast<uintptr_t>(lengths) & 7u) == 0, "tg_gru_seq_forward: lengths must be 8-byte aligned (int64)");
    hipStream_t s = (hipStream_t)stream;
    const StepGrid g = step_grid(B, H, D);
    const long gi_ds = (long)B * T * 3 * H, save_ds = (long)B * T * 5 * H;
    for (int step = 0; step < T; ++step)
        hipLaunchKernelGGL(gru_seq_fwd_step_kernel, g.grid, dim3(GRU_THREADS), 0, s, gi, gi_ds, w_hh_fwd, w_hh_rev, b_hh_fwd, b_hh_rev, h0,
                           (const long long*)lengths, y, h_n, save, save_ds, (int*)flag, B, T, H, D, step, g.n_jt, g.n_bt);
    return check_launch("tg_gru_seq_forward");
}

extern "C" int tg_gru_seq_backward(const float* dy, const float* dh_n, const float* save, const float* w_hh_t_fwd, const float* w_hh_t_rev,
                                   const void* lengths, float* dgi, float* dgh, float* dh0, float* dh_scratch, int32_t B, int32_t T, int32_t H,
                                   int32_t D, void* stream) {
    TG_REQUIRE(gru_seq_in_envelope(B, T, H, D), "tg_gru_seq_backward: outside the envelope " GS_ENVELOPE " (B=%d T=%d H=%d D=%d)", B, T, H, D);
    TG_REQUIRE(dy && save && w_hh_t_fwd && dgi && dgh && dh_scratch && (D == 1 || w_hh_t_rev), "tg_gru_seq_backward: null pointer");
    TG_REQUIRE(aligned16(w_hh_t_fwd) && aligned16(w_hh_t_rev) && aligned16(dgh), "tg_gru_seq_backward: w_hh_t / dgh must be 16-byte aligned");
    TG_REQUIRE(!lengths || (reinterpret_cast<uintptr_t>(lengths) & 7u) == 0, "tg_gru_seq_backward: lengths must be 8-byte aligned (int64)");
    hipStream_t s = (hipStream_t)stream;
    const StepGrid g = step_grid(B, H, D);
    const long save_ds = (long)B * T * 5 * H, dg_ds = (long)B * T * 3 * H;
    const int steps = dh0 ? T + 1 : T;    // the extra step forms dh0 of the rows of full length (shorter rows form theirs on the way)
    for (int step = 0; step < steps; ++step)
        hipLaunchKernelGGL(gru_seq_bwd_step_kernel, g.grid, dim3(GRU_THREADS), 0, s, dy, dh_n, save, save_ds, w_hh_t_fwd, w_hh_t_rev,
                           (const long long*)lengths, dgi, dgh, dg_ds, dh_scratch, dh0, B, T, H, D, step, g.n_jt, g.n_bt);
    return check_launch("tg_gru_seq_backward");
}
