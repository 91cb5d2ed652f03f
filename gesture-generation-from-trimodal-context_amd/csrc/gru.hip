// Bidirectional GRU recurrence (nn.GRU semantics) on the f32 matrix cores.
//
// Two regimes, both without any in-kernel inter-workgroup synchronisation (nothing can dead-lock):
//
//  * H = 300 (generator): the recurrent product h_{t-1}[B,H] x W_hh^T[H,3H] is too large for one CU's LDS + registers
//    (W_hh fp32 = 1.08 MB per direction), so each time step is ONE launch covering both directions, every batch tile
//    and every 16-wide slice of hidden units; the launch boundary (~1.5 us) is the grid-wide dependency, cheaper than
//    an in-kernel grid barrier (4-7 us on 256 CUs).  The step's workgroup tiling, product and gate epilogue: gru_step.hpp.  h_t goes
//    straight into the layer output y, which doubles as the state store.
//
//  * H = 64 (discriminator): persistent kernels with W_hh in registers, see gru_h64.hip.
#include "gru_step.hpp"    // the workgroup tiling, the product and the cell (shared with gru_seq.hip)

namespace tg {

__global__ __launch_bounds__(GRU_THREADS) void gru_fwd_step_kernel(
    const float* __restrict__ gi, long gi_ds, const float* __restrict__ whh0, const float* __restrict__ whh1,
    const float* __restrict__ bhh0, const float* __restrict__ bhh1, float* __restrict__ Y, float* __restrict__ save,
    long save_ds, int B, int T, int H, int step, int n_jt, int n_bt) {
    __shared__ float red[GRU_KS][GRU_MT][3][4][64];
    const StepTile t = step_tile(n_jt, n_bt);
    const int dir = t.dir, erow = t.erow, ej = t.ej;
    const int tau = dir ? T - 1 - step : step;
    const int tau_prev = dir ? tau + 1 : tau - 1;
    const bool has_prev = step > 0;
    const float* bhh = dir ? bhh1 : bhh0;

    // the gate epilogue's operands do not depend on the product, so their loads go out first
    const bool e_ok = erow < B && ej < H;
    float gi_r = 0.f, gi_z = 0.f, gi_n = 0.f, hp = 0.f, bh_r = 0.f, bh_z = 0.f, bh_n = 0.f;
    if (e_ok) {
        const float* gip = gi + dir * gi_ds + ((long)erow * T + tau) * (3 * H);
        gi_r = gip[ej]; gi_z = gip[H + ej]; gi_n = gip[2 * H + ej];
        bh_r = bhh[ej]; bh_z = bhh[H + ej]; bh_n = bhh[2 * H + ej];
        if (has_prev) hp = Y[((long)erow * T + tau_prev) * (2 * H) + dir * H + ej];
    }

    const bool b_ok = t.brow < B;
    const float* hrow = Y + ((long)(b_ok ? t.brow : 0) * T + tau_prev) * (2 * H) + dir * H;
    float gh[3];
    step_product_fwd(has_prev, hrow, b_ok, dir ? whh1 : whh0, H, t, red, gh);
    if (!e_ok) return;
    const GruCell c = gru_cell_fwd(gi_r, gi_z, gi_n, gh, bh_r, bh_z, bh_n, hp);
    Y[((long)erow * T + tau) * (2 * H) + dir * H + ej] = c.h;
    if (save) {
        float* sp = save + dir * save_ds + ((long)erow * T + tau) * (4 * H);
        sp[ej] = c.r; sp[H + ej] = c.z; sp[2 * H + ej] = c.n; sp[3 * H + ej] = c.hn;
    }
}

// Backward step at time tau (the reverse of the forward order).  Using the gate gradients dgh of the step that
// consumed h_tau (tau_next, written by the previous launch):
//     dh_tau = dy_tau + dh_next * z_next + dgh_next @ W_hh        (W_hh passed transposed: [H][3H])
// then this step's own gate gradients for the 16 hidden units the workgroup owns (gru_cell_bwd):
//     dgi = [dr, dz, dn]   dgh = [dr, dz, dn * r]
__global__ __launch_bounds__(GRU_THREADS) void gru_bwd_step_kernel(
    const float* __restrict__ dY, const float* __restrict__ Y, const float* __restrict__ save, long save_ds,
    const float* __restrict__ wt0, const float* __restrict__ wt1, float* __restrict__ dgi, float* __restrict__ dgh, long dg_ds,
    float* __restrict__ dhbuf, int B, int T, int H, int step, int n_jt, int n_bt) {
    __shared__ float red[GRU_KS][GRU_MT][4][64];
    const StepTile t = step_tile(n_jt, n_bt);
    const int dir = t.dir, erow = t.erow, ej = t.ej;
    const int tau = dir ? step : T - 1 - step;
    const int tau_next = dir ? tau - 1 : tau + 1;   // consumer of h_tau in forward order
    const int tau_prev = dir ? tau + 1 : tau - 1;   // producer of h_prev for this cell
    const bool has_next = step > 0;
    const bool has_prev = dir ? (tau < T - 1) : (tau > 0);
    const int H3 = 3 * H;

    // epilogue operands (independent of the product): issue their loads first
    const bool e_ok = erow < B && ej < H;
    float dy = 0.f, r = 0.f, z = 0.f, n = 0.f, hn = 0.f, hp = 0.f, z_next = 0.f, dh_next = 0.f;
    float* dh_w = dhbuf + ((long)(step & 1) * 2 + dir) * (long)B * H;
    const float* dh_r = dhbuf + ((long)((step & 1) ^ 1) * 2 + dir) * (long)B * H;
    if (e_ok) {
        dy = dY[((long)erow * T + tau) * (2 * H) + dir * H + ej];
        const float* sp = save + dir * save_ds + ((long)erow * T + tau) * (4 * H);
        r = sp[ej]; z = sp[H + ej]; n = sp[2 * H + ej]; hn = sp[3 * H + ej];
        if (has_prev) hp = Y[((long)erow * T + tau_prev) * (2 * H) + dir * H + ej];
        if (has_next) {
            z_next = save[dir * save_ds + ((long)erow * T + tau_next) * (4 * H) + H + ej];
            dh_next = dh_r[(long)erow * H + ej];
        }
    }

    const bool b_ok = t.brow < B;
    const float* arow = dgh + dir * dg_ds + ((long)(b_ok ? t.brow : 0) * T + tau_next) * H3;
    const float s = step_product_bwd(has_next, arow, b_ok, dir ? wt1 : wt0, H, t, red);
    if (!e_ok) return;
    float dh = dy;
    if (has_next) dh += s + dh_next * z_next;
    const GruCellGrad g = gru_cell_bwd(dh, r, z, n, hn, hp);
    const long o = dir * dg_ds + ((long)erow * T + tau) * H3 + ej;
    store_gate_grads(dgi + o, dgh + o, H, g.dr, g.dz, g.dn, g.dn * r);
    dh_w[(long)erow * H + ej] = dh;
}

}  // namespace tg

using namespace tg;

constexpr int HS = 64;      // H = 64 runs in the persistent kernels of gru_h64.hip

extern "C" int tg_gru_forward(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev,
                              const float* b_hh_fwd, const float* b_hh_rev, float* y, float* save, int64_t save_dir_stride,
                              int32_t B, int32_t T, int32_t H, void* stream) {
    TG_REQUIRE(gi && w_hh_fwd && w_hh_rev && b_hh_fwd && b_hh_rev && y, "tg_gru_forward: null pointer");
    TG_REQUIRE(B > 0 && T > 0 && H > 0 && H % 4 == 0, "tg_gru_forward: need H %% 4 == 0 (H=%d)", H);
    TG_REQUIRE(aligned16(w_hh_fwd) && aligned16(w_hh_rev) && aligned16(y), "tg_gru_forward: w_hh / y must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (H == HS)
        return tg_gru_h64_forward(gi, gi_dir_stride, w_hh_fwd, w_hh_rev, b_hh_fwd, b_hh_rev, y, save, save_dir_stride, nullptr, nullptr, B, T,
                                  stream);
    const StepGrid g = step_grid(B, H, 2);
    for (int step = 0; step < T; ++step)
        hipLaunchKernelGGL(gru_fwd_step_kernel, g.grid, dim3(GRU_THREADS), 0, s, gi, (long)gi_dir_stride, w_hh_fwd,
                           w_hh_rev, b_hh_fwd, b_hh_rev, y, save, (long)save_dir_stride, B, T, H, step, g.n_jt, g.n_bt);
    return check_launch("tg_gru_forward");
}

extern "C" int tg_gru_backward(const float* dy, const float* y, const float* save, int64_t save_dir_stride,
                               const float* w_hh_t_fwd, const float* w_hh_t_rev, float* dgi, float* dgh, int64_t dg_dir_stride,
                               float* dh_scratch, int32_t B, int32_t T, int32_t H, void* stream) {
    TG_REQUIRE(dy && y && save && w_hh_t_fwd && w_hh_t_rev && dgi && dgh && dh_scratch, "tg_gru_backward: null pointer");
    TG_REQUIRE(B > 0 && T > 0 && H > 0 && H % 4 == 0, "tg_gru_backward: need H %% 4 == 0 (H=%d)", H);
    TG_REQUIRE(aligned16(w_hh_t_fwd) && aligned16(w_hh_t_rev) && aligned16(dgh) && (dg_dir_stride % 4 == 0),
               "tg_gru_backward: w_hh_t / dgh must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (H == HS)
        return tg_gru_h64_backward(dy, nullptr, y, save, save_dir_stride, w_hh_t_fwd, w_hh_t_rev, dgi, dgh, dg_dir_stride, B, T, stream);
    const StepGrid g = step_grid(B, H, 2);
    for (int step = 0; step < T; ++step)
        hipLaunchKernelGGL(gru_bwd_step_kernel, g.grid, dim3(GRU_THREADS), 0, s, dy, y, save, (long)save_dir_stride,
                           w_hh_t_fwd, w_hh_t_rev, dgi, dgh, (long)dg_dir_stride, dh_scratch, B, T, H, step, g.n_jt, g.n_bt);
    return check_launch("tg_gru_backward");
}
