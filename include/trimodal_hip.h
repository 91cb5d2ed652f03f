/*
 * trimodal_hip.h -- C ABI of libtrimodal_hip.so (gfx950 / MI355X kernels for the trimodal gesture GAN path).
 *
 * The reference (ai4r/Gesture-Generation-from-Trimodal-Context) has no FFI: its hot path is PyTorch
 * nn.Modules whose arithmetic runs in ATen.  Each entry point below replaces the ATen
 * kernel behind one reference call site; the call site is cited per function as file:line relative to
 * /root/reference/scripts/.  INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only: device pointers, sizes, a hipStream_t passed as void*.
 *   - every function returns 0 on success, non-zero on error; tg_last_error() gives the message
 *     (thread-local).  No C++ exception crosses the ABI.
 *   - all device memory is owned by the caller.  Functions never allocate, never synchronise the device
 *     and are safe to call during hipGraph stream capture.
 *   - all tensors are fp32, row-major, "channel-last" for sequences: (batch, time, channels).
 *   - functions documented "accumulates" add into their output; the caller zeroes it when needed.
 */
#ifndef TRIMODAL_HIP_H
#define TRIMODAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_ABI_VERSION 11

int tg_version(void);

/* Deterministic mode (ABI 5).  Scope: the GAN TRAINING ITERATION (train_eval/train_gan.py:13-103 as train_gan.GanTrainer issues it).
 * on != 0: every combine across workgroups on that path runs in a fixed order -- weight-gradient splits through the two-pass
 * fp64 reduce (the caller passes a workspace for every problem and takes bias gradients through tg_colsum), embedding scatters with one
 * writer per table row, the discriminator head's parameter gradients and tg_colsum by one workgroup, BatchNorm partial sums in thread order --
 * so two runs from the same state give bit-identical results (the reference on CPU is reproducible given a seed; float atomics are not).
 * The fused discriminator front-end backward (tg_d_preconv_bwd) and the fused speaker backward (tg_speaker_bwd) combine by float atomics and
 * are not to be called in this mode (the host mirror takes their generic forms).  Process-wide, like tg_set_math_mode.
 * NOT covered (they keep their atomics whatever the mode): the autoencoder path (tg_ae_train_step's fp64 BatchNorm / loss sums, tg_ae_loss),
 * tg_l1_mean and the single-launch BatchNorm statistics kernels for tensors under 16 K elements (tg_bn_train_stats / tg_bn_backward: fp64
 * atomics, whose order-dependence is below fp32 resolution but not zero).  tests/test_trajectory_gpu.py pins the guarantee at B = 64. */
int tg_set_deterministic(int32_t on);
int tg_get_deterministic(void);
/* Workgroup cap of the persistent weight-gradient kernel (tg_gemm_tn / tg_gemm_tn_group on the mover-wave kernel; process-wide, 0 = none):
 * with n > 0 those launches are planned for, and occupy, at most n CUs -- for a launch issued on a second stream BESIDE a kernel that needs
 * the other CUs to itself (the cluster-synchronised GRU backward keeps 160 of 256; train_eval/train_gan.py:89 is the backward it belongs
 * to).  A group the capped plan cannot take is refused by tg_gemm_tn_kernel_plan (code 0) exactly as without the cap; callers check that
 * before they fork. */
int tg_set_tn_workgroup_cap(int32_t n);
int tg_get_tn_workgroup_cap(void);
const char* tg_last_error(void);

/* Math mode of the GEMM-shaped kernels (process-wide, like cublasSetMathMode):
 *   0 (default): fp32-accurate products, parity with the reference to ~1e-6.  Small products run on the f32 matrix cores
 *      (v_mfma_f32_16x16x4_f32, exact fp32 fma chains); the big forward / input-gradient products (tg_gemm_nt, M >= 1024) split
 *      each fp32 operand exactly into three bf16 terms and accumulate the six significant partial products in fp32 on the
 *      bf16 matrix cores (csrc/gemm_split.hip): same error as the f32 path, 1.2-1.8x its speed.  Environment TG_GEMM_X3=0
 *      keeps everything on the f32 matrix cores.
 *   1: those big products round their operands to bf16 (RNE) instead, one MFMA per product, fp32 accumulate; everything in HBM
 *      stays fp32, weight gradients and the recurrences stay fp32.  The precision BASELINE.json configs[1] names; tolerance
 *      2e-2 forward / 5e-2 gradients. */
int tg_set_math_mode(int32_t mode);
int tg_get_math_mode(void);

/*
 * A "row window" view of a channel-last activation buffer: the A operand of every GEMM-shaped op.
 * Logical matrix element (m, k), m in [0, M), k in [0, K):
 *     b  = m / rows_out,  r = m % rows_out            (clip b, output row r inside the clip)
 *     kk = k / cw,        c = k % cw                  (tap kk, channel c)
 *     sr = r * row_step + shift + kk * dil            (source row inside the clip)
 *     value = (0 <= sr < rows_in) ? ptr[b * batch_stride + sr * row_stride + c] : 0
 * A plain matrix is {rows_out = rows_in = M, row_step = 1, shift = 0, cw = K}.  A Conv1d(kernel kw, stride s,
 * padding p, dilation d) over (B, L, C) is {cw = C, K = kw*C, row_step = s, shift = -p, dil = d}: im2col is never
 * materialised.
 */
typedef struct tg_window {
    const float* ptr;
    int64_t batch_stride;
    int64_t row_stride;
    int32_t rows_in;
    int32_t rows_out;
    int32_t row_step;
    int32_t shift;
    int32_t dil;
    int32_t cw;
    int32_t K;
} tg_window;

/* ---- GEMM-shaped ops (f32 MFMA v_mfma_f32_16x16x4_f32, exact fp32 accumulate) ------------------------------
 * tg_gemm_nt: C(m, n) = act( sum_k A(m,k) * Bw[n*ldb + k] + bias[n] ) (+ C(m,n) when accumulate != 0)
 *   act(x) = x >= 0 ? x : act_slope * x   (1.0 = identity, 0.0 = ReLU, 0.3/0.2 = LeakyReLU)
 *   C row m is stored at C + (m / c_rows_out) * c_batch_stride + (m % c_rows_out) * c_row_stride.
 *   Replaces nn.Linear / nn.Conv1d / nn.ConvTranspose1d forward and their input-gradients:
 *   model/multimodal_context_net.py:13-22,51,89-93,100-104,214-220,225-226; model/tcn.py:19,25;
 *   the x @ W_ih^T half of nn.GRU (:98,223); model/embedding_net.py:24,48-62,187-206. */
typedef struct tg_gemm_nt_problem {
    tg_window A;
    const float* Bw;
    int64_t ldb;
    int32_t b_seg_k;           /* 0: one weight matrix.  > 0 (a divisor of K): K-concatenated weights, k in [s*b_seg_k, (s+1)*b_seg_k) */
    int32_t reserved;          /*    reads Bw + s*b_seg_stride + n*ldb + (k - s*b_seg_k) -- e.g. both GRU directions' W_ih^T side by side */
    int64_t b_seg_stride;
    const float* bias;
    float* C;
    int64_t c_batch_stride, c_row_stride;
    int32_t c_rows_out, M, N;
    float act_slope;
    int32_t accumulate;
    const float* out_scale;    /* NULL, or an element-wise multiplier applied after the activation, addressed like C: the inverted-dropout
                                  scale mask of F.dropout(relu(conv(x))) (model/tcn.py:22-29) rides in the epilogue */
    const void* b_planes;      /* NULL, or Bw PRE-SPLIT: plane 0 of a slab-tiled bf16 x 3 plane buffer (see tg_split3_planes below) of b_rows rows */
    int64_t b_plane_stride;    /*   and K columns whose rows b_row0 .. b_row0 + N - 1 are Bw's (planes b_plane_stride elements apart; one weight */
    int32_t b_rows, b_row0;    /*   matrix only: b_seg_k == 0).  Many-row products then run on the mover-wave kernel (csrc/gemm_mw.hip): the weights go
                                    global -> LDS by DMA, only the activation is split while staged.  Ignored by the other kernels (Bw is still read). */
    /* Epilogue extensions (big-product path only, tg_gemm_nt_ext_supported): what the reference computes right after the product in
     * model/tcn.py:27-45 without another pass over the tensor.  All three are addressed like C.
     *   gate : the result (after act / out_scale) is kept where gate > 0 and zeroed elsewhere -- ReLU backward through the tensor the
     *          product's consumer saw (the chain rule of relu + dropout of the PREVIOUS conv, applied to this input gradient);
     *   res, C2 (together): second output C2 = act2(C_new + res), act2 = leaky-ReLU of slope res_slope (0: ReLU) -- the residual
     *          block's relu(out + x) written next to out, which the backward still needs. */
    const float* gate;
    const float* res;
    float* C2;
    float res_slope;
    /* ABI 4 -- the dropout scale REGENERATED instead of read (no mask tensor, no draw launch): with drop_state != NULL (out_scale must be
     * NULL) the multiplier of the element at offset o from C (in elements, o as C is addressed) is element drop_index0 + o of the draw
     * tg_dropout_mask(mask, n, drop_p, drop_state, drop_site) would write -- Philox4x32-10 keyed by the element index, so forward and
     * backward consumers of one F.dropout (model/tcn.py:22-29) see the same mask without storing it.  Needs the big-product path
     * (tg_gemm_nt_ext_supported), a vectorisable C and drop_index0 % 4 == 0; refused with an error elsewhere. */
    uint32_t drop_site;
    const uint64_t* drop_state;
    int64_t drop_index0;
    float drop_p;
    int32_t reserved4;
    /* ABI 7 -- fp16 x 2 operands (three matrix instructions per product instead of bf16 x 3's six, csrc/common.hpp "two-term fp16 split"):
     * b_planes_kind == 1 says b_planes is the TWO-plane fp16 buffer tg_split2h_planes writes (hi / lo of every row scaled by its own power of
     * two) and b_inv_scale its per-row inverse scales (b_rows + 1 floats, 16-byte aligned, b_row0 % 4 == 0); a_row_scale (or a_rowmax, below) then holds the
     * power-of-two scale of every product row m < M of the window A (M floats, tg_h2_row_scales: the row's largest magnitude over its K values
     * scaled into [2^14, 2^15)) by which the kernel multiplies the row before splitting it.  b_planes_kind == 0: bf16 x 3
     * planes as before, both pointers ignored.  Same arithmetic contract as before: fp32 nn.Linear / nn.Conv1d / nn.GRU input projections
     * (model/multimodal_context_net.py:98-104, model/tcn.py:19-25) within the fp32 tolerance. */
    int32_t b_planes_kind;
    int32_t reserved5;
    const float* b_inv_scale;
    const float* a_row_scale;
    /* ... or, for windows of one or two taps, a_rowmax: the largest magnitude of every SOURCE row of A's tensor (index batch * rows_in + source row,
     * non-negative floats: tg_win_row_absmax, or the product that wrote the tensor through c_rowmax below); the kernel derives the product rows'
     * scales from it.  Exactly one of a_row_scale / a_rowmax with fp16 x 2 planes.
     * c_rowmax / c2_rowmax (optional, mover-wave kernel only -- refused elsewhere): M floats each; row m's entry is raised (atomic unsigned max on the
     * float's bits) to the largest magnitude the product wrote into row m of C / C2.  The caller zeroes them before the first product of a pass;
     * a chain of convs (model/tcn.py:27-46) then needs no separate pass over an activation to scale it. */
    const float* a_rowmax;
    float* c_rowmax;
    float* c2_rowmax;
    int32_t a_rowmax_rows;     /* 0 / 1: a_rowmax has one entry per source row; n > 1: one entry per n consecutive source rows (entry (batch * rows_in +
                                  source row) / n) -- e.g. one per clip of T frames, as tg_gru_backward_cluster_stats leaves them */
    int32_t reserved6;
} tg_gemm_nt_problem;
/* tg_gemm_nt_group: up to 8 independent tg_gemm_nt products in ONE launch (both GRU directions' input projections, the stride
 * phases of a conv input-gradient ...).  All problems must fall into the same kernel family as problem 0 (big / narrow / small);
 * outputs must not overlap.  The table is copied into the kernel arguments: nothing has to outlive the call. */
int tg_gemm_nt_group(const tg_gemm_nt_problem* problems, int32_t n, void* stream);
/* kernel family a problem would run in (0 big, 1 narrow N <= 32, 2 small; -1 invalid): problems of one group must agree */
int32_t tg_gemm_nt_family(const tg_gemm_nt_problem* problem);
/* 1 when this problem would run on a kernel that implements gate / res / C2 (family 0 on the bf16 x 3 or bf16 path), else 0 */
int32_t tg_gemm_nt_ext_supported(const tg_gemm_nt_problem* problem);
/* Which kernel a group of n problems would run on, without launching: 0 = f32-MFMA / narrow / small kernels (gemm.hip),
 * 1 = bf16 x 3 staged-slab kernel (gemm_split.hip), 2 = bf16 x 3 mover-wave kernel (gemm_mw.hip: 512-thread workgroups, big tiles,
 * chosen when its tiles fill the chip); -1 invalid.  *tile_m / *tile_n (may be NULL) receive the workgroup tile for plan 2.
 * Replaces nothing in the reference (torch picks its own GEMM there, multimodal_context_net.py:98-99, model/tcn.py:19-46): test
 * and profiling aid, so that a parity test can assert WHICH kernel it covered. */
int32_t tg_gemm_nt_kernel_plan(const tg_gemm_nt_problem* problems, int32_t n, int32_t* tile_m, int32_t* tile_n);
/* Which instantiation of the no-LDS f32-MFMA kernel (gemm.hip, families 1 and 2) a group would run on, without launching -- the choice
 * tg_gemm_nt_group itself makes from the group's workgroup count, largest K and largest M.  Returns the family (0, 1, 2) or -1 (invalid,
 * mixed families, or operands these kernels refuse); for families 1 and 2 fills out = {family, vec (16-byte loads), wm, wn (waves per
 * workgroup: tile 32 wm x 32 wn), ring (k-steps of operands in flight), ks (waves splitting K: 1 or 4)}; family 0 fills nothing.
 * Test aid like tg_gemm_nt_kernel_plan: a parity test asserts which kernel it covered. */
int32_t tg_gemm_nt_variant(const tg_gemm_nt_problem* problems, int32_t n, int32_t out[6]);
/* Which instantiation of the staged-slab bf16 x 3 kernel (gemm_split.hip: gemm_nt_split_kernel) a big-product group would run on, without
 * launching -- the choice tg_gemm_nt_group itself makes.  Returns 1 and fills out = {tile rows (128 / 64), tile columns (96 / 64), db (1: two
 * LDS buffers), fast (1: the addressing form without row masks, every window of the group free of padding)} for a group that
 * tg_gemm_nt_kernel_plan answers with 1; -1 for any other plan or an invalid group (out untouched).  Test aid like tg_gemm_nt_variant. */
int32_t tg_gemm_nt_split_variant(const tg_gemm_nt_problem* problems, int32_t n, int32_t out[4]);
/* Process-wide switch of the mover-wave kernel: 1 on, 0 off (every big product on gemm_split.hip), -1 back to the environment default
 * (TG_NT_MW, on).  For same-process A/B timing (tools/nt_mw_probe.py) and tests; results are equal within the fp32 tolerance either way. */
int tg_set_nt_mover_waves(int32_t on);
int tg_gemm_nt(const tg_window* A, const float* Bw, int64_t ldb, const float* bias, float* C,
               int64_t c_batch_stride, int64_t c_row_stride, int32_t c_rows_out, int32_t M, int32_t N,
               float act_slope, int32_t accumulate, void* stream);

/* ---- pre-split operand planes (csrc/planes.hip).  Plane buffer of an fp32 matrix [rows][cw]: three bf16 planes (x = hi + mid + lo exactly)
 * `plane_stride` ELEMENTS apart, each SLAB-TILED: [cwp / 32][rows + 1][32] (cwp = cw rounded up to a multiple of 32; element (r, c) at
 * ((c / 32) * (rows + 1) + r) * 32 + c % 32; zero past cw and in row `rows` of every slab), so that one 32-deep K slab of 16 consecutive rows
 * is 1 KB of contiguous memory.  tg_gemm_nt_problem.b_planes takes weights in this form (mover-wave kernel, csrc/gemm_mw.hip). */
int tg_split3_planes(const float* x, int64_t ldx, int32_t rows, int32_t cw, void* planes, int32_t cwp, int64_t plane_stride, void* stream);
/* fp16 x 2 form of the same buffer (ABI 7): TWO fp16 planes, same slab tiling, holding hi = fp16(x s_r), lo = fp16(x s_r - hi) with s_r the
 * power of two that puts row r's largest magnitude into [2^14, 2^15); inv_scale[r] = 1 / s_r for r < rows, 0 for the zero row (rows + 1 floats).
 * Weights of nn.GRU / weight-normed nn.Conv1d as the matrix cores' fp16 operand (multimodal_context_net.py:98-99, model/tcn.py:19-25). */
int tg_split2h_planes(const float* x, int64_t ldx, int32_t rows, int32_t cw, void* planes, int32_t cwp, int64_t plane_stride, float* inv_scale, void* stream);
/* The same planes for the K-CONCATENATED TRANSPOSE of two [rows][cols] matrices: plane row n < cols, column k < 2 rows holds w{k / rows}[k % rows][n]
 * (cwp >= 2 rows; inv_scale: cols + 1 floats) -- the weight operand of the GRU layer's input gradient dx = [dgi_fwd | dgi_rev] @ [W_ih_fwd ; W_ih_rev]
 * as one product over K = 6H, straight from the two weight_ih parameters (nn.GRU backward, model/multimodal_context_net.py:98-99). */
int tg_split2h_planes_tcat(const float* w0, const float* w1, int32_t rows, int32_t cols, void* planes, int32_t cwp, int64_t plane_stride, float* inv_scale,
                           void* stream);
/* rowmax[b * A->rows_in + r] = max_c |A->ptr[b * batch_stride + r * row_stride + c]|, c < A->cw, for b < batches, r < A->rows_in: the largest magnitude
 * of every SOURCE row of a window operand (one pass over the tensor; several windows over one tensor share it). */
int tg_win_row_absmax(const tg_window* A, int32_t batches, float* rowmax, void* stream);
/* row_scale[m] = 2^(141 - e_m), e_m the biased fp32 exponent (clamped to [32, 250]) of the largest magnitude among the K values of product row m of
 * the window A -- tg_gemm_nt_problem.a_row_scale.  src_rowmax == NULL: read from the tensor itself (a row with t taps is read t times);
 * else from tg_win_row_absmax's output for that tensor (batch b = m / rows_out, source rows (m % rows_out) * row_step + shift + tap * dil). */
int tg_h2_row_scales(const tg_window* A, int32_t M, const float* src_rowmax, float* row_scale, void* stream);
/* One pass over an fp32 matrix x[M][C] (row stride ldx): rowmax[m] = largest magnitude of row m (M floats, or NULL); colmax[g * C + c] = largest
 * magnitude of column c within row group g (the M rows cut into `groups` equal consecutive parts, e.g. the two directions of a GRU layer's gate
 * gradients [2][B * T][3H]; groups * C floats, or NULL).  colmax is zeroed and then raised by atomic unsigned max.  Feeds a_rowmax of
 * tg_gemm_nt_problem and y_colmax / a_colmax of tg_gemm_tn_problem when the tensor's producer does not supply them. */
int tg_absmax_rows_cols(const float* x, int64_t ldx, int32_t M, int32_t C, int32_t groups, float* rowmax, float* colmax, void* stream);

/* tg_gemm_tn (weight gradient, accumulates): dW[n*ldw + perm(k)] += sum_m dY[m*ldy + n] * A(m, k).
 *   out_kw == 0: perm(k) = k.  out_kw == K/cw: perm(k) = (k % cw) * out_kw + k / cw, i.e. the gradient lands in
 *   the (Cout, Cin, kw) layout of nn.Conv1d weights.
 *   The sum over m is split across workgroups.  ws == NULL: partial tiles are combined with f32 atomics (order
 *   varies run to run).  ws != NULL (>= tg_gemm_tn_ws_floats(M, N, K) floats): partials of <= 512 rows go to ws and are
 *   combined in split order in fp64 -- bitwise reproducible, and accurate for the ~1e6-row sums of the audio encoder.
 *   Replaces the weight-gradient half of aten::convolution_backward / addmm backward for the same call sites. */
int64_t tg_gemm_tn_ws_floats(int32_t M, int32_t N, int32_t K);
/*   dbias != NULL: also dbias[n] += sum_m dY[m*ldy + n] (the bias gradient rides along; no separate pass over dY). */
typedef struct tg_gemm_tn_problem {
    const float* dY;
    int64_t ldy;
    tg_window A;
    float* dW;
    int64_t ldw;
    int32_t M, N, out_kw, reserved;
    float* dbias;
    float* ws;
    int64_t ws_floats;
    /* ABI 7 -- fp16 x 2 operands on the mover-wave kernel (both non-NULL, 16-byte aligned; ignored by the other kernels, which read the fp32
     * operands): y_colmax[n] = largest magnitude of column n of dY over the M rows (N floats), a_colmax[c] = largest magnitude of channel c of A's
     * tensor (cw floats, valid for every tap) -- tg_absmax_rows_cols or the kernels that wrote the tensors.  The sum runs over rows, so each
     * COLUMN is scaled by its own power of two; the combine scales the sums back.  Same contract: the weight-gradient half of
     * aten::convolution_backward / addmm backward within the fp32 tolerance. */
    const float* y_colmax;
    const float* a_colmax;
} tg_gemm_tn_problem;
/* tg_gemm_tn_group: up to 8 independent weight gradients in ONE launch (the four of a GRU layer: W_ih / W_hh of both directions). */
int tg_gemm_tn_group(const tg_gemm_tn_problem* problems, int32_t n, void* stream);
/* which kernel the group would run on, without launching: 0 = f32-MFMA tiles, 1 = bf16 x 3 staged slabs (gemm_split.hip), 2 = bf16 x 3 mover
 * waves (gemm_tn_mw.hip: persistent 768-thread workgroups, 192 x 160 tiles); -1 invalid.  Test / profiling aid like tg_gemm_nt_kernel_plan. */
int32_t tg_gemm_tn_kernel_plan(const tg_gemm_tn_problem* problems, int32_t n);
/* tg_gemm_tn_kernel_plan's answer, and for plans 0 and 1 every problem's row-split plan as launched (n entries each, any may be NULL):
 * splits, rows_per_split (a multiple of 32; the last split may be shorter) and reduce_kind -- 0: float atomics (ws == NULL), 16 / 256: the
 * fixed-order fp64 combine with that many threads per output entry (256 from 512 splits on).  Plan 2 fills nothing.  Test aid. */
int32_t tg_gemm_tn_split_plan(const tg_gemm_tn_problem* problems, int32_t n, int32_t* splits, int32_t* rows_per_split, int32_t* reduce_kind);
/* The dW tile of the staged-slab bf16 x 3 weight-gradient kernel (gemm_split.hip: gemm_tn_split_kernel<tnw, tkw>, tile 32 tnw x 32 tkw) as
 * tg_gemm_tn_group chooses it: returns 1 and fills out = {tnw, tkw} for a group tg_gemm_tn_kernel_plan answers with 1, -1 otherwise (out
 * untouched).  Test aid. */
int32_t tg_gemm_tn_split_tile(const tg_gemm_tn_problem* problems, int32_t n, int32_t out[2]);
int tg_gemm_tn(const float* dY, int64_t ldy, const tg_window* A, float* dW, int64_t ldw, int32_t M, int32_t N,
               int32_t out_kw, float* dbias, float* ws, int64_t ws_floats, void* stream);

/* tg_colsum (bias gradient): out[n] (+)= sum_m X[m*ldx + n]. */
int tg_colsum(const float* X, int64_t ldx, int32_t M, int32_t N, float* out, int32_t accumulate, void* stream);

/* ---- GRU recurrence (nn.GRU, batch_first, bidirectional; model/multimodal_context_net.py:98-99,155,223-224,241)
 * gi   : [2][B][T][3H] input projections x@W_ih^T + b_ih per direction (dir stride in floats given explicitly)
 * y    : [B][T][2H]    layer output; direction d writes columns [d*H, (d+1)*H); also the recurrent state store
 * save : [2][B][T][4H] r, z, n, (W_hn h + b_hn) per step for the backward pass, or NULL (inference / no-grad)
 * Gate order and maths are PyTorch's: r,z = sigmoid, n = tanh(gi_n + r*(W_hn h + b_hn)), h' = (1-z) n + z h.
 * H != 64: one launch per time step (both directions, all batch rows); the launch boundary is the grid-wide dependency.
 * H == 64: one persistent launch for the whole sequence (tg_gru_h64_forward without the fused dropout). */
int tg_gru_forward(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev,
                   const float* b_hh_fwd, const float* b_hh_rev, float* y, float* save, int64_t save_dir_stride,
                   int32_t B, int32_t T, int32_t H, void* stream);

/* Backward through time.  dy: [B][T][2H] gradient w.r.t. y.  w_hh_t_*: TRANSPOSED recurrent weights [H][3H].
 * Outputs dgi, dgh: [2][B][T][3H] gradients w.r.t. the input-side and hidden-side gate pre-activations
 * (feed tg_gemm_tn / tg_gemm_nt / tg_colsum for dW_ih, dW_hh, dx, db).  dh_scratch: 4*B*H floats. */
int tg_gru_backward(const float* dy, const float* y, const float* save, int64_t save_dir_stride,
                    const float* w_hh_t_fwd, const float* w_hh_t_rev, float* dgi, float* dgh, int64_t dg_dir_stride,
                    float* dh_scratch, int32_t B, int32_t T, int32_t H, void* stream);

/* H = 64 recurrence (the discriminator's GRU): one persistent launch per layer, recurrent product on the bf16 matrix cores at
 * fp32 accuracy (csrc/gru_h64.hip).  Same tensors as tg_gru_forward / tg_gru_backward plus the fused inter-layer dropout of
 * nn.GRU(dropout=p):
 *   forward : drop_mask [B][T][128] (inverted-dropout scale mask, 0 or 1/(1-p)) and y_drop [B][T][128] -- both or neither;
 *             y_drop = y * drop_mask is the next layer's input (y itself stays the recurrent state / backward operand).
 *   backward: dy_mask [B][T][128] or NULL: the incoming gradient is multiplied by it while it is loaded (the gradient w.r.t.
 *             y_drop becomes the gradient w.r.t. y).  No dh_scratch: the carried dh stays in registers. */
int tg_gru_h64_forward(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev,
                       const float* b_hh_fwd, const float* b_hh_rev, float* y, float* save, int64_t save_dir_stride,
                       const float* drop_mask, float* y_drop, int32_t B, int32_t T, void* stream);
int tg_gru_h64_backward(const float* dy, const float* dy_mask, const float* y, const float* save, int64_t save_dir_stride,
                        const float* w_hh_t_fwd, const float* w_hh_t_rev, float* dgi, float* dgh, int64_t dg_dir_stride,
                        int32_t B, int32_t T, void* stream);

/* Persistent, cluster-synchronised variant of tg_gru_forward for H <= 320 (the generator): ONE launch walks all T
 * steps of both directions; the workgroups that share a batch tile exchange h_t through `ws` with write-through stores and
 * per-workgroup flag words, no grid-wide barrier (csrc/gru_cluster.hip).  Same arguments and results as tg_gru_forward.
 * ws: tg_gru_cluster_ws_bytes(B, H) bytes of device memory, 16-byte aligned, ZERO-FILLED ONCE by the caller when allocated and
 * then left to the library: the flag words behind the timeout block are numbered by a per-cluster generation that persists from
 * launch to launch (no fill kernel per launch; re-zeroing the WHOLE workspace between launches is allowed, part of it is not).  Its
 * first 16 words are a sticky TIMEOUT block: word 0 is set by the kernel if a bounded spin expires (results are then invalid),
 * words 1.. hold diagnostics.  No launch ever clears them -- a timeout in any launch sharing the workspace stays visible until
 * the caller reads word 0 back (after synchronising) and clears it itself.
 * tg_gru_cluster_supported(B, H) != 0 iff the launch fits co-resident at one workgroup per CU on the current device (its CU
 * count is queried: B <= 384 at H = 300 on the 256 CUs of an unpartitioned MI355X; 0 under CPX/DPX partitions that are too small). */
int32_t tg_gru_cluster_supported(int32_t B, int32_t H);
int64_t tg_gru_cluster_ws_bytes(int32_t B, int32_t H);
/* drop_mask / y_drop ([B][T][2H], both or neither; need tg_gru_cluster_fused_dropout() != 0): the inter-layer dropout of
 * nn.GRU(dropout=p) rides in the kernel's output stage, y_drop = y * drop_mask is the next layer's input. */
int32_t tg_gru_cluster_fused_dropout(void);
int tg_gru_forward_cluster(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev,
                           const float* b_hh_fwd, const float* b_hh_rev, float* y, float* save, int64_t save_dir_stride,
                           const float* drop_mask, float* y_drop, void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H, void* stream);
/* The same, saving the gates only for batch rows [save_row0, save_row0 + save_rows): of the stacked generator calls of a GAN iteration
 * (train_gan.py:30,50,67) only one is differentiated; the other rows of `save` are left untouched. */
int tg_gru_forward_cluster_rows(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev,
                                const float* b_hh_fwd, const float* b_hh_rev, float* y, float* save, int64_t save_dir_stride,
                                const float* drop_mask, float* y_drop, void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H,
                                int32_t save_row0, int32_t save_rows, void* stream);

/* Inference recurrence for a handful of sequences (1 <= B <= 4, 64 < H <= 320): the single-utterance synthesis window of
 * scripts/synthesize.py:131-160 (one 34-frame window per generator call; multimodal_context_net.py:155, nn.GRU bidirectional, eval mode: no
 * saved gates, no dropout).  h_t is exchanged as fp32 words that are their own flags (sentinel-polled), the product is fp32 FMAs on resident
 * fp32 weights: no operand split at all, results at fp32 rounding of the reference's (csrc/gru_vec.hip).  Same operand layout as
 * tg_gru_forward.  Workspace: tg_gru_vec_ws_bytes(H) bytes whose first tg_gru_vec_ws_header_bytes() are ZERO and every byte behind them 0xFF
 * before the first use (and again after a timeout: word 0 is the sticky timeout word of tg_gru_forward_cluster's convention). */
int32_t tg_gru_vec_supported(int32_t B, int32_t H);
int64_t tg_gru_vec_ws_bytes(int32_t H);
int32_t tg_gru_vec_ws_header_bytes(void);
int tg_gru_forward_vec(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                       const float* b_hh_rev, float* y, void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H, void* stream);
/* The one-direction form of the same kernel (ContextEncoder's GRU of the joint-embedding baseline, embedding_net.py:233): gi [B][T][3H],
 * w_hh [3H][H] (16-byte aligned), b_hh [3H], y [B][T][H]; no h0, no lengths.  Envelope as tg_gru_vec_supported: 1 <= B <= 4, 64 < H <= 320,
 * H % 4 == 0, T >= 1; outside it the entry returns non-zero ("unsupported shape ... envelope" in tg_last_error) and launches nothing;
 * tg_gru_vec1_supported writes 1 / 0 for a shape of positive sizes.  A WORKSPACE BELONGS TO ONE DIRECTION COUNT: a launch resets only the
 * words of its own directions in the other launch buffer, so a workspace used by tg_gru_forward_vec1 must never be handed to
 * tg_gru_forward_vec or the other way round (size and initial fill are the same: tg_gru_vec_ws_bytes(H)). */
int tg_gru_vec1_supported(int32_t B, int32_t H, int32_t* supported);
int tg_gru_forward_vec1(const float* gi, const float* w_hh, const float* b_hh, float* y, void* ws, int64_t ws_bytes, int32_t B, int32_t T,
                        int32_t H, void* stream);
/* The constant-input form of the same kernel, for a layer whose input is the same row at every time step (PoseDecoderGRU's layer 0,
 * embedding_net.py:153-157): gi [n_dir][B][3H] is ONE projected row per sequence and direction (gi_dir_stride floats between the directions,
 * at least B * 3H; ignored with n_dir = 1) and is used at all T steps; y [B][T][n_dir * H]; w_hh_rev / b_hh_rev are ignored with n_dir = 1.
 * Same arithmetic as the time-varying entries on that row repeated T times: y is bit-identical.  Envelope: that of tg_gru_vec_supported and
 * n_dir in {1, 2}, T >= 1; outside it the entry returns non-zero ("unsupported shape ... envelope" in tg_last_error) and launches nothing;
 * tg_gru_vec_const_supported writes 1 / 0 for positive sizes.  WORKSPACE: the rule of one direction count per workspace holds, and the
 * constant-input form MAY SHARE a workspace with the time-varying form of the same direction count (tg_gru_forward_vec for n_dir = 2,
 * tg_gru_forward_vec1 for n_dir = 1): grid, slot layout, resets and the launch counter are the same code, only the gi address differs. */
int tg_gru_vec_const_supported(int32_t B, int32_t H, int32_t n_dir, int32_t* supported);
int tg_gru_forward_vec_const(const float* gi, int64_t gi_dir_stride, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd,
                             const float* b_hh_rev, float* y, void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H, int32_t n_dir,
                             void* stream);

/* Persistent cluster-synchronised variant of tg_gru_backward (B <= 192 at H = 300; no dh_scratch: the carried dh stays in
 * registers).  Same workspace / timeout-word convention as tg_gru_forward_cluster. */
int32_t tg_gru_cluster_bwd_supported(int32_t B, int32_t H);
int64_t tg_gru_cluster_bwd_ws_bytes(int32_t B, int32_t H);
/* dy_mask ([B][T][2H] or NULL): multiplied into dy while it is loaded (the backward of the fused dropout). */
int tg_gru_backward_cluster(const float* dy, const float* dy_mask, const float* y, const float* save, int64_t save_dir_stride,
                            const float* w_hh_t_fwd, const float* w_hh_t_rev, float* dgi, float* dgh, int64_t dg_dir_stride,
                            void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H, void* stream);
/* The same launch, also leaving the magnitudes of what it wrote for the fp16 x 2 products that read dgi / dgh next (ABI 7; all three or none, zeroed
 * by the caller, raised by atomic unsigned max when the kernel leaves, so row chunks of one pass accumulate): gi_rowmax[dir * rowmax_dir_stride + b] =
 * largest |dgi| of batch row b over its T steps (a_rowmax of the input-gradient product dx = dgi @ W_ih with a_rowmax_rows = T: one scale per
 * clip), gi_colmax / gh_colmax[dir * 3H + c] = largest |dgi| / |dgh| of column c
 * (y_colmax of the weight-gradient products).  Replaces nothing in the reference beyond tg_gru_backward_cluster's nn.GRU backward
 * (model/multimodal_context_net.py:98-99). */
int tg_gru_backward_cluster_stats(const float* dy, const float* dy_mask, const float* y, const float* save, int64_t save_dir_stride,
                                  const float* w_hh_t_fwd, const float* w_hh_t_rev, float* dgi, float* dgh, int64_t dg_dir_stride,
                                  void* ws, int64_t ws_bytes, int32_t B, int32_t T, int32_t H, float* gi_rowmax, int64_t rowmax_dir_stride,
                                  float* gi_colmax, float* gh_colmax, void* stream);

/* ---- BatchNorm1d, channel-last [rows][C] (model/multimodal_context_net.py:14,17,20,215,218) -------------
 * Training statistics per group: the rows are split into `groups` equal consecutive slabs, each normalised with
 * its own batch statistics (several reference forward calls stacked into one launch); running stats are updated
 * once per group in order (momentum 0.1, unbiased variance), num_batches_tracked += groups * repeats.
 * repeats >= 1: the running update of each group is applied that many times (the same batch seen by `repeats`
 * identical reference forward calls: the three generator forwards of one GAN iteration share their audio input).
 * ws: 2*groups*C doubles of scratch.  mean/rstd: [groups][C] outputs. */
int tg_bn_train_stats(const float* x, int32_t rows, int32_t C, int32_t groups, double* ws, float* mean, float* rstd,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float eps,
                      float momentum, int32_t repeats, void* stream);
/* eval mode: mean/rstd from running stats. */
/* Small tensors (the discriminator's and the autoencoder's BatchNorms): statistics, running-stat update AND y = act(gamma * xhat +
 * beta) in ONE single-workgroup launch; y == NULL computes the statistics only.  tg_bn_fused_supported: rows * C <= 2^19, C a
 * multiple of 4 that divides 4096 (16-byte accesses with fixed channels per thread); x / y 16-byte aligned. */
int32_t tg_bn_fused_supported(int32_t rows, int32_t C, int32_t groups);
int tg_bn_train_fused(const float* x, float* y, int32_t rows, int32_t C, int32_t groups, float* mean, float* rstd,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                      const float* beta, float act_slope, float eps, float momentum, int32_t repeats, void* stream);
int tg_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps, float* mean,
                     float* rstd, void* stream);
/* y = act((x - mean[g]) * rstd[g] * gamma + beta). */
int tg_bn_apply(const float* x, float* y, int32_t rows, int32_t C, int32_t groups, const float* mean,
                const float* rstd, const float* gamma, const float* beta, float act_slope, void* stream);
/* backward of act(BN(x)) for one group: dx, and dgamma/dbeta (accumulate).  ws: 2*C doubles.
 * mean==NULL selects eval-mode backward is not supported (training only). */
int tg_bn_backward(const float* dy, const float* x, float* dx, int32_t rows, int32_t C, const float* mean,
                   const float* rstd, const float* gamma, const float* beta, float act_slope, double* ws,
                   float* dgamma, float* dbeta, void* stream);

/* Two-launch forms for tensors past the single-workgroup size: x [groups * rows_per_group][C] holds `groups` stacked forward calls, each
 * normalised with its own batch statistics (mean / rstd [groups][C]); no zero fill, no atomics, deterministic.  ws: tg_bn2_ws_doubles
 * doubles of scratch.  tg_bn2_train: statistics, running-stat updates in call order (each `repeats` times) and y = act(BN(x)) (y may be
 * NULL: statistics only); tg_bn2_backward: dx for all groups and dgamma / dbeta += the groups' sums (either may be NULL).
 * Supported: C a multiple of 4 that divides 256, rows_per_group * C a multiple of 4, 16-byte aligned pointers. */
int32_t tg_bn2_supported(int32_t rows_per_group, int32_t C);
int64_t tg_bn2_ws_doubles(int32_t rows_per_group, int32_t C, int32_t groups);
int tg_bn2_train(const float* x, float* y, int32_t rows_per_group, int32_t C, int32_t groups, double* ws, int64_t ws_doubles, float* mean,
                 float* rstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                 const float* beta, float act_slope, float eps, float momentum, int32_t repeats, void* stream);
int tg_bn2_backward(const float* dy, const float* x, float* dx, int32_t rows_per_group, int32_t C, int32_t groups, const float* mean,
                    const float* rstd, const float* gamma, const float* beta, float act_slope, double* ws, int64_t ws_doubles,
                    float* dgamma, float* dbeta, void* stream);

/* ---- ConvDiscriminator.pre_conv, train-mode forward in ONE launch (model/multimodal_context_net.py:214-220: Conv1d(27,16,3) -> BN(16) ->
 * LeakyReLU(True) = identity -> Conv1d(16,8,3) -> BN(8) -> identity -> Conv1d(8,8,3); poses [Bs][34][27] channel-last, `groups` stacked
 * forward calls with their own batch statistics).  Writes what the separate launches write: the conv outputs c1 [Bs][32][16], c2 [Bs][30][8],
 * c3 [Bs][28][8], the BatchNorm outputs y1 / y2 (same shapes as c1 / c2), mean / rstd [groups][C], and updates the running statistics in call
 * order (either pair may be NULL).  ws: tg_d_preconv_ws_bytes(Bs) bytes, 16-byte aligned, ZERO before the first use and left zero by every
 * launch (workgroups of one launch meet at two device-wide barriers: one launch at a time per workspace; a timeout sets ws[0], sticky). */
int32_t tg_d_preconv_fwd_supported(int32_t Bs, int32_t groups);
int64_t tg_d_preconv_ws_bytes(int32_t Bs);
int tg_d_preconv_fwd(const float* poses, const float* w1, const float* b1, const float* gamma1, const float* beta1, const float* w2,
                     const float* b2, const float* gamma2, const float* beta2, const float* w3, const float* b3, float* c1, float* y1,
                     float* c2, float* y2, float* c3, float* mean1, float* rstd1, float* mean2, float* rstd2, float* running_mean1,
                     float* running_var1, int64_t* nbt1, float* running_mean2, float* running_var2, int64_t* nbt2, void* ws,
                     int64_t ws_bytes, int32_t Bs, int32_t groups, float eps, float momentum, void* stream);

/* The same block backwards in ONE launch: dc3 [nb][28][8] = gradient at the GRU input; the forward's tensors of the same nb clips (whole
 * statistics groups; mean / rstd of exactly those groups); parameter gradients ACCUMULATE (float atomics) -- the ten pointers are all given
 * or all NULL; dposes (NULL, or [nb][34][27]) receives the pose gradient, added to its content when dposes_accumulate.  Same workspace rule. */
int tg_d_preconv_bwd(const float* dc3, const float* poses, const float* c1, const float* y1, const float* c2, const float* y2,
                     const float* mean1, const float* rstd1, const float* mean2, const float* rstd2, const float* w1, const float* w2,
                     const float* w3, const float* gamma1, const float* gamma2, float* dw1, float* db1, float* dgamma1, float* dbeta1,
                     float* dw2, float* db2, float* dgamma2, float* dbeta2, float* dw3, float* db3, float* dposes,
                     int32_t dposes_accumulate, void* ws, int64_t ws_bytes, int32_t nb, int32_t groups, void* stream);

/* ---- speaker / style path (model/multimodal_context_net.py:83-95,125-137; embedding_net.py:10-13), fused ------------------------------
 * forward: se = table[vid], zc = W1 se + b1, mu = Wmu zc + bmu, logvar = Wlv zc + blv, z = mu + eps * exp(0.5 logvar) (all [B][16]); with
 * rep != NULL also rep[(b * T + t) * rep_ld + j] = z[b][j] (the style columns of the GRU input).  eps is read when rng_state == NULL and
 * WRITTEN otherwise (ABI 4): drawn as tg_normal(eps, B * 16, rng_state, site) would, in the same launch (torch.randn_like of :92).
 * backward (nb <= tg_speaker_bwd_max_rows()): dz [nb][16] = gradient w.r.t. z; d_mu_in / d_logvar_in: direct gradients or NULL; every
 * parameter gradient accumulates; dtable rows meet in float atomics. */
int tg_speaker_fwd(const float* table, const int64_t* vid, int32_t n_rows, const float* w1, const float* b1, const float* wmu, const float* bmu,
                   const float* wlv, const float* blv, float* eps, float* se, float* zc, float* mu, float* logvar, float* z,
                   int32_t B, float* rep, int64_t rep_ld, int32_t T, const uint64_t* rng_state, uint32_t site, void* stream);
int32_t tg_speaker_bwd_max_rows(void);
int tg_speaker_bwd(const float* dz, const float* d_mu_in, const float* d_logvar_in, const float* logvar, const float* eps, const float* zc,
                   const float* se, const int64_t* vid, int32_t n_rows, const float* w1, const float* wmu, const float* wlv, float* dw1,
                   float* db1, float* dwmu, float* dbmu, float* dwlv, float* dblv, float* dtable, int32_t nb, void* stream);

/* ---- output MLP Linear(H, Hm) -> LeakyReLU(True) (== identity, reference README.md:122) -> Linear(Hm, D), as ONE linear map -------------
 * (model/multimodal_context_net.py:100-104,157-158).  _compose: w21 [D][dup H] = W2 W1 (written dup = 1 or 2 times side by side), w21t
 * [dup H][D] its transpose (may be NULL), b21 = W2 b1 + b2.  dup = 2 lets the map act on the bidirectional GRU output [fwd | rev] without the
 * direction sum (:155-156) being formed.  _param_grads: from P [D][dup H] = d_out^T o (dup = 2: its halves are added) and s [D] =
 * colsum(d_out): dW1 += W2^T P, db1 += W2^T s, dW2 += P W1^T + s b1^T, db2 += s. */
int tg_out_mlp_compose(const float* w1, const float* b1, const float* w2, const float* b2, int32_t H, int32_t Hm, int32_t D, int32_t dup,
                       float* w21, float* w21t, float* b21, void* stream);
int tg_out_mlp_param_grads(const float* P, const float* s, const float* w1, const float* b1, const float* w2, int32_t H, int32_t Hm, int32_t D,
                           int32_t dup, float* dw1, float* db1, float* dw2, float* db2, void* stream);

/* ---- WavEncoder front end: Conv1d(1, 16, 15, stride, padding) -> BatchNorm1d(16) -> LeakyReLU, fused ------------------------
 * Replaces feat_extractor[0..2] of model/multimodal_context_net.py:13-15 (and their autograd backward) without materialising the
 * pre-BatchNorm tensor: the convolution is recomputed from the raw audio wherever it is needed (csrc/audio.hip).
 * audio: B clips of L samples, `audio_stride` floats apart; w [16][15], bias [16]; T1 = (L + 2 pad - 15) / stride + 1 output frames.
 * ws: scratch of tg_wav_front_ws_doubles() doubles (no initialisation needed); fstat: tg_wav_front_fstat_doubles() doubles written by
 * _stats and read by _backward (sums of the forward pass); gate: tg_wav_front_gate_words(B, T1) 64-bit words written by _apply
 * (one bit per output element: pre-activation > 0, so act'(0) = act_slope as in tg_bn_backward) and read by _backward. */
int64_t tg_wav_front_ws_doubles(void);
int64_t tg_wav_front_fstat_doubles(void);
int64_t tg_wav_front_gate_words(int32_t B, int32_t T1);
/* train-mode batch statistics of the conv output over all B * T1 frames: mean / rstd [16], running statistics updated `repeats` times
 * (momentum form of nn.BatchNorm1d), num_batches_tracked += repeats.  running_* / num_batches_tracked / fstat may be NULL. */
int tg_wav_front_stats(const float* audio, int64_t audio_stride, int32_t B, int32_t L, const float* w, const float* bias, int32_t stride,
                       int32_t pad, int32_t T1, double* ws, int64_t ws_doubles, float* mean, float* rstd, float* running_mean,
                       float* running_var, int64_t* num_batches_tracked, double* fstat, float eps, float momentum, int32_t repeats,
                       void* stream);
/* y [B][T1][16] = act((conv - mean) * rstd * gamma + beta) (mean / rstd from _stats, or tg_bn_eval_stats in eval mode); gate may be NULL. */
int tg_wav_front_apply(const float* audio, int64_t audio_stride, int32_t B, int32_t L, const float* w, const float* bias, int32_t stride,
                       int32_t pad, int32_t T1, const float* mean, const float* rstd, const float* gamma, const float* beta, float act_slope,
                       float* y, uint64_t* gate, void* stream);
/* backward of the block for d y = dact [B][T1][16]: dW [16][15], dbias, dgamma, dbeta accumulate (each may be NULL); the input is raw
 * audio, so no input gradient. */
int tg_wav_front_backward(const float* dact, const uint64_t* gate, const float* audio, int64_t audio_stride, int32_t B, int32_t L, const float* w,
                          const float* bias, int32_t stride, int32_t pad, int32_t T1, const float* mean, const float* rstd, const float* gamma,
                          const double* fstat, float act_slope, double* ws, int64_t ws_doubles, float* dW, float* dbias, float* dgamma,
                          float* dbeta, void* stream);

/* The same backward with the input gradient of the NEXT layer, Conv1d(16, 32, 15, stride 6) (feat_extractor[3], weight w2 [32][16][15]),
 * computed on the fly from dc2 [B][T2][32] = the gradient w.r.t. that conv's output: d act is never materialised. */
int tg_wav_front_backward_fused(const float* dc2, int32_t T2, const float* w2, const uint64_t* gate, const float* audio, int64_t audio_stride,
                                int32_t B, int32_t L, const float* w, const float* bias, int32_t stride, int32_t pad, int32_t T1,
                                const float* mean, const float* rstd, const float* gamma, const double* fstat, float act_slope, double* ws,
                                int64_t ws_doubles, float* dW, float* dbias, float* dgamma, float* dbeta, void* stream);

/* Weight and bias gradient of feat_extractor[3] = Conv1d(16, 32, 15, stride 6): dW2 [32][16][15] += sum dc2[b, q, co] act[b, 6 q + k, ci],
 * db2 [32] += sum dc2 (either may be NULL); act [B][T1][16], dc2 [B][T2][32], T2 = (T1 - 15) / 6 + 1.  ws: tg_wav_conv2_wgrad_ws_floats()
 * floats of scratch.  One pass over the activation, deterministic. */
int64_t tg_wav_conv2_wgrad_ws_floats(void);
int tg_wav_conv2_wgrad(const float* dc2, const float* act, int32_t B, int32_t T1, int32_t T2, float* ws, int64_t ws_floats, float* dW2,
                       float* db2, void* stream);

/* ---- element-wise / data movement ------------------------------------------------------------------- */
/* y = max(a + b, 0)  (model/tcn.py:46);  dx = dy * (y > 0). */
int tg_add_relu(const float* a, const float* b, float* y, int64_t n, void* stream);
/* both gates of a residual block's backward in one pass: dsum = dy * (y > 0); dc = dsum * (o > 0 ? 1 : slope) * mask (mask may be NULL) */
int tg_act_mask_bwd2(const float* dy, const float* y, const float* o, const float* mask, float slope, float* dsum, float* dc, int64_t n, void* stream);
/* dx = dy * mask * (y > 0 ? 1 : slope); mask may be NULL (=1).  Backward of act() followed by dropout. */
int tg_act_mask_bwd(const float* dy, const float* y, const float* mask, float slope, float* dx, int64_t n,
                    void* stream);
/* The same two with the dropout scale REGENERATED: the multiplier of element i is element index0 + i of the draw
 * tg_dropout_mask(mask, n, p, rng_state, site) would write (see tg_gemm_nt_problem.drop_state).  n and index0 multiples of 4, 16-byte
 * aligned pointers.  model/tcn.py:22-29 backward without a stored mask. */
int tg_act_mask_bwd_drop(const float* dy, const float* y, float p, const uint64_t* rng_state, uint32_t site, int64_t index0, float slope,
                         float* dx, int64_t n, void* stream);
int tg_act_mask_bwd2_drop(const float* dy, const float* y, const float* o, float p, const uint64_t* rng_state, uint32_t site, int64_t index0,
                          float slope, float* dsum, float* dc, int64_t n, void* stream);
/* y = x * mask  (nn.Dropout with a materialised inverted-dropout mask: 0 or 1/(1-p)). */
int tg_mul(const float* x, const float* mask, float* y, int64_t n, void* stream);
/* y (+)= alpha * x. */
/* Zero `bytes` (multiple of 4) at p with a kernel of this library (graph-capture safe; the library never uses hipMemsetAsync:
 * captured memset nodes were observed to replay with a clobbered fill pattern on ROCm 7.2, see csrc/common.hpp). */
int tg_zero(void* p, int64_t bytes, void* stream);
int tg_axpy(const float* x, float* y, float alpha, int32_t accumulate, int64_t n, void* stream);
/* dst[r*ldd + c] (+)= src[r*lds + c], r < rows, c < cols. */
int tg_copy2d(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t rows, int32_t cols,
              int32_t accumulate, void* stream);
/* dst[(b*T + t)*ldd + c] = src[b*lds + c]  (z repeated over time, multimodal_context_net.py:151-153). */
int tg_repeat_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t B, int32_t T, int32_t cols,
                   void* stream);
/* dst[b*ldd + c] (+)= sum_t src[(b*T + t)*lds + c]. */
int tg_sum_rows(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t B, int32_t T, int32_t cols,
                int32_t accumulate, void* stream);
/* o[m*H + j] = y[m*2H + j] + y[m*2H + H + j]  (multimodal_context_net.py:156,242). */
int tg_add_halves(const float* y, float* o, int32_t M, int32_t H, void* stream);
/* out[i] = sum_q parts[q * stride + i], i < n (n, stride multiples of 4; 16-byte aligned): K-split partial products combined in a fixed order. */
int tg_sum_parts(const float* parts, int64_t stride, int32_t n_parts, float* out, int64_t n, void* stream);
/* out [M][8] = a0 [M][K] . w0 [K][8] + a1 [M][K] . w1 [K][8] (K % 4 == 0, contiguous operands, 16-byte aligned a0 / a1): the input gradient of a
 * bidirectional GRU layer with 8 input channels, dx = dgi_fwd W_ih_fwd + dgi_rev W_ih_rev (the discriminator's nn.GRU(8, 64), :222-223). */
int tg_narrow8_pair(const float* a0, const float* a1, const float* w0, const float* w1, float* out, int32_t M, int32_t K, void* stream);
/* dy[m*2H + j] = dy[m*2H + H + j] = do[m*H + j]. */
int tg_dup_halves(const float* d_o, float* dy, int32_t M, int32_t H, void* stream);
/* pre[b][t][:D] = t < n_pre ? target[b][t][:] : 0 ; pre[b][t][D] = t < n_pre  (train_eval/train_gan.py:20-22). */
int tg_make_pre_seq(const float* target, float* pre, int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream);
/* Batch assembly on the device (ABI 5): SpeechMotionDataset.__getitem__ after the LMDB read (data_loader/lmdb_data_loader.py:107-171) and
 * default_collate_fn's stacking (:43-53) for B clips in one launch, from RAW per-clip records.
 *   audio_raw / audio_off [B + 1]: the stored audio of the clips back to back, clip b = [audio_off[b], audio_off[b + 1]) (any length);
 *   vec_raw / vec_off [B + 1] (offsets in floats): the stored direction vectors, at least n_poses frames per clip; n_ext [B] or NULL: the stored
 *   frame count vec_seq.shape[0] of each sample (NULL: (vec_off[b + 1] - vec_off[b]) / pose_floats, i.e. the whole sequence was shipped);
 *   word_idx / word_onset [B][Wmax], n_words [B]: vocabulary index (lang_model.get_word_index, resolved on the host) and onset time of each word;
 *   times [B][2]: aux_info start_time, end_time; vid_in [B] or NULL: speaker index (train.py:178-183).
 * Writes in_text [B][n_poses] (extend_word_seq :115-140, fp64 as the reference's doubles; remove_word_timing != 0: words evenly spread),
 * in_audio [B][audio_len] (utils/data_utils.py:68-74: truncate or numpy 'symmetric' padding), target [B][n_poses][pose_floats]
 * (vec_seq[0:n_poses]) and vid [B] -- bit for bit what the host path produces. */
int tg_assemble_batch(const float* audio_raw, const int64_t* audio_off, const float* vec_raw, const int64_t* vec_off, const int64_t* word_idx,
                      const double* word_onset, const int32_t* n_words, const double* times, const int32_t* n_ext, const int64_t* vid_in, int32_t B, int32_t Wmax,
                      int32_t n_poses, int32_t pose_floats, int32_t audio_len, int32_t remove_word_timing, int64_t* out_text, float* out_audio,
                      float* out_vec, int64_t* out_vid, void* stream);
/* out[i*D + :] = table[idx[i]*D + :]  (nn.Embedding, multimodal_context_net.py:40,89). */
int tg_embed_gather(const float* table, const int64_t* idx, float* out, int32_t n_idx, int32_t D, int32_t n_rows,
                    void* stream);
/* The look-up followed by F.dropout(p) (multimodal_context_net.py:47-52, train mode) in one pass: out = table[idx] * mask, mask = the draw
 * tg_dropout_mask(mask, n_idx * D, p, rng_state, site) would write; it is not stored -- the backward regenerates it (tg_act_mask_bwd_drop with
 * slope 1).  D % 4 == 0, 16-byte aligned table and out. */
int tg_embed_gather_drop(const float* table, const int64_t* idx, float* out, int32_t n_idx, int32_t D, int32_t n_rows, float p,
                         const uint64_t* rng_state, uint32_t site, void* stream);
/* The text encoder's TCN forward (model/tcn.py:16-46, multimodal_context_net.py:57-61) as ONE clip-local launch (csrc/tcn_fused.hip):
 * x0 [clips][T][C] (the embedding-dropout output) -> n_blocks TemporalBlocks (two weight-normed causal convs of kernel 2, dilation 2^i, each
 * + ReLU + dropout p, then relu(out + x)) -> Linear(C, 32) written to out + (clip * T + t) * out_ld.  Envelope: T = 34, C = 300, n_blocks = 4,
 * fp32-accurate math mode.  w_planes / w_inv: the fp16 x 2 planes (tg_split2h_planes) of the 2 n_blocks packed conv weights stacked as
 * [w_rows = 2 n_blocks C][2 C], planes w_plane_stride elements apart; biases: 2 n_blocks pointers to C floats.  Dropout: element
 * j * clips * T * C + i of the draw tg_dropout_mask(.., p, rng_state, site) would write scales element i of conv j's output (not stored;
 * rng_state may be null when p == 0).  o0 / o1 / y: [n_blocks][clips][T][C] each (conv1 output, conv2 output, block output, post-dropout);
 * only the clips [save_row0, save_row0 + save_rows) are written (save_rows == 0: nothing, the three may be null).  16-byte aligned operands. */
int tg_tcn_fwd_fused(const float* x0, const void* w_planes, int64_t w_plane_stride, int32_t w_rows, const float* w_inv, const float* const* biases,
                     const float* dec_w, const float* dec_b, const uint64_t* rng_state, uint32_t site, float p, int32_t clips, int32_t T, int32_t C,
                     int32_t n_blocks, float* o0, float* o1, float* y, int32_t save_row0, int32_t save_rows, float* out, int64_t out_ld,
                     void* stream);
/* dtable[idx[i]*D + :] += dout[i*D + :]  (dense embedding gradient; accumulates). */
int tg_embed_scatter_add(const float* dout, const int64_t* idx, float* dtable, int32_t n_idx, int32_t D,
                         int32_t n_rows, void* stream);
/* out[perm-ed] = in: generic 3-D permute, out[i0][i1][i2] with out dims (d[p0], d[p1], d[p2]) of in dims d. */
int tg_permute3(const float* in, float* out, int32_t d0, int32_t d1, int32_t d2, int32_t p0, int32_t p1,
                int32_t p2, void* stream);

/* One launch for a table of independent tg_permute3 jobs (all weight transposes / conv packs of a network after an optimiser
 * step).  desc: device array of n_jobs x 10 int64 = {src, dst, d0, d1, d2, p0, p1, p2, first_workgroup, workgroup_count}; jobs
 * sorted by first_workgroup, total_workgroups = sum of the counts.  Same element mapping as tg_permute3. */
int tg_permute3_batch(const int64_t* desc, int32_t n_jobs, int32_t total_workgroups, void* stream);
/* Weight pack for the input-gradient of Conv1d(stride s) (= forward of ConvTranspose1d):
 * w: [Co][Ci][kw] -> out: [s][Ci][J][Co], J = ceil(kw/s), out[r][ci][j][co] = (r + s*j < kw) ? w[co][ci][r + s*j] : 0.
 * Phase r serves the input positions p with (p % s) == r:  dx[6q + r] = sum_j dy[q - j] . out[r][:, j, :]. */
int tg_conv_dgrad_pack(const float* w, float* out, int32_t Co, int32_t Ci, int32_t kw, int32_t s, void* stream);

/* ---- weight norm (torch.nn.utils.weight_norm dim=0; model/tcn.py:19,25) ------------------------------
 * v: [Co][Ci][kw], g: [Co].  w_packed: [Co][kw][Ci] = g * v / ||v||  (tap-major, the layout tg_gemm_nt wants). */
int tg_weight_norm_fwd(const float* v, const float* g, float* w_packed, int32_t Co, int32_t Ci, int32_t kw,
                       void* stream);
/* All weight-normed convs of a network in ONE launch (same Co, Ci, kw): w_packed[i] as tg_weight_norm_fwd, and -- when w_t != NULL --
 * w_t[i] = the same weight as [Ci][kw*Co] (w_t[ci][tap*Co + co]), the B operand of the conv's input gradient. */
int tg_weight_norm_fwd_batch(int32_t n, const float* const* v, const float* const* g, float* const* w_packed, float* const* w_t,
                             int32_t Co, int32_t Ci, int32_t kw, void* stream);
/* dw_packed: [Co][kw][Ci] -> dg[Co], dv[Co][Ci][kw] (both accumulate). */
int tg_weight_norm_bwd(const float* dw_packed, const float* v, const float* g, float* dg, float* dv, int32_t Co,
                       int32_t Ci, int32_t kw, void* stream);
/* The same for n <= 8 convs of equal shape in one launch (tables of n pointers). */
int tg_weight_norm_bwd_batch(int32_t n, const float* const* dw_packed, const float* const* v, const float* const* g, float* const* dg,
                             float* const* dv, int32_t Co, int32_t Ci, int32_t kw, void* stream);

/* ---- randomness: Philox4x32-10 counter RNG, graph-replay safe -----------------------------------------
 * rng_state: device uint64[2] = {seed, step}.  tg_rng_advance bumps step by one (launch once per iteration).
 * Every draw site passes its own `site` id so streams never collide. */
int tg_rng_advance(uint64_t* rng_state, void* stream);
/* start of a training iteration in one launch: rng_state[1] += 1 for up to two RNG states and += 1 for up to two Adam step counters
 * (tg_adam_step then runs with the counter already advanced); any pointer may be NULL, not all. */
int tg_iter_begin(uint64_t* rng_a, uint64_t* rng_b, int32_t* adam_step_a, int32_t* adam_step_b, void* stream);
/* The head of one train_iter_gan call (scripts/train_eval/train_gan.py:13-30,50,67-72) in ONE launch: tg_iter_begin's counters; the seed
 * poses of the `copies` stacked generator calls (tg_make_pre_seq, pre_stacked [copies][B][T] rows of D + 1 floats, pre_ld floats apart:
 * pre_ld > D + 1 writes them straight into the pose columns of the GRU input rows); the word ids copied `copies` times
 * (text [B][T] -> text_stacked, both may be NULL); the speaker ids [vid] * (copies - 1) + [last] (vid [B] -> vid_stacked [copies][B], both
 * may be NULL) where last = vid[perm] if permute_last -- perm = torch.randperm(B) of :69 drawn as tg_randperm(.., rng_a at its NEW step,
 * perm_site) or given (perm_in, tests), also written to perm_out when non-NULL -- and vid otherwise.  B <= 1024 with speaker ids.
 * target_copy (ABI 5; NULL, or [B][T][D]): receives a copy of target -- the "real" half of the discriminator's stacked input, so that
 * torch.cat((target, out_dir_vec.detach())) of :30-31 needs no launch of its own (the generator writes its half behind it). */
int tg_iter_head(uint64_t* rng_a, uint64_t* rng_b, int32_t* adam_step_a, int32_t* adam_step_b, const float* target, float* pre_stacked, int64_t pre_ld,
                 int32_t B, int32_t T, int32_t D, int32_t n_pre, int32_t copies, const int64_t* text, int64_t* text_stacked, const int64_t* vid,
                 int64_t* vid_stacked, int32_t permute_last, const int64_t* perm_in, uint32_t perm_site, int64_t* perm_out, float* target_copy,
                 void* stream);
int tg_dropout_mask(float* mask, int64_t n, float p, const uint64_t* rng_state, uint32_t site, void* stream);
/* Draw the same mask and apply it in one pass: mask as tg_dropout_mask, y[i] = x[i] * mask[i] (F.dropout, train mode).  mask may be NULL
 * (ABI 4): the mask is not stored, its later consumers regenerate it (tg_gemm_nt_problem.drop_state, tg_act_mask_bwd_drop). */
int tg_dropout_apply(const float* x, float* y, float* mask, int64_t n, float p, const uint64_t* rng_state, uint32_t site,
                     void* stream);
int tg_normal(float* out, int64_t n, const uint64_t* rng_state, uint32_t site, void* stream);
/* out = random permutation of [0, n), n <= 1024 (torch.randperm at train_eval/train_gan.py:62). */
int tg_randperm(int64_t* out, int32_t n, const uint64_t* rng_state, uint32_t site, void* stream);
/* out[i] = src[perm[i]] for int64 vectors (vid_indices[rand_idx], train_gan.py:63). */
int tg_gather_i64(const int64_t* src, const int64_t* perm, int64_t* out, int32_t n, void* stream);

/* ---- speaker path (multimodal_context_net.py:128-131; model/embedding_net.py:10-13) -------------------- */
/* z = mu + eps * exp(0.5 * logvar) */
int tg_reparam_fwd(const float* mu, const float* logvar, const float* eps, float* z, int64_t n, void* stream);
/* dmu += dz ; dlogvar += dz * eps * 0.5 * exp(0.5*logvar) */
int tg_reparam_bwd(const float* dz, const float* logvar, const float* eps, float* dmu, float* dlogvar, int64_t n,
                   void* stream);

/* ---- losses (train_eval/train_gan.py:41,53-89) ----------------------------------------------------------
 * Discriminator step.  logit_*: pre-sigmoid outputs [B].  out[0] = dis_error; d_logit_* = d dis_error / d logit. */
int tg_gan_d_loss(const float* logit_real, const float* logit_fake, int32_t B, float* out, float* d_logit_real,
                  float* d_logit_fake, void* stream);
/* Generator step.  out_pose/target/out_rand: [B][T*D]; z, z_rand, mu, logvar: [B][Z]; logit_out: [B] (pre-sigmoid
 * D(out)).  scalars[0..4] = huber, kld, div_reg, gen_error, total loss (unweighted terms; total is weighted).
 * Gradients of the TOTAL loss: d_out [B][T*D], d_mu, d_logvar [B][Z] (written), d_logit_out [B] (0 when
 * use_gan == 0).  ws: 3*B floats. */
int tg_gan_g_loss(const float* out_pose, const float* target, const float* out_rand, const float* z,
                  const float* z_rand, const float* mu, const float* logvar, const float* logit_out, int32_t B,
                  int32_t TD, int32_t Z, float w_huber, float w_kld, float w_div, float w_gan, int32_t use_gan,
                  float* ws, float* scalars, float* d_out, float* d_mu, float* d_logvar, float* d_logit_out,
                  void* stream);
/* ConvDiscriminator head (multimodal_context_net.py:243-252) in one launch each way.  y: [B][T][2H] last GRU layer output;
 * w1/b1: out (Linear H -> 1), w2/b2: out2 (Linear T -> 1).  forward: l1 [B][T] per-frame logits (kept for the backward), logit [B]
 * (pre-sigmoid), prob [B].  backward: d_logit [B] -> dy [B][T][2H]; dw1/db1/dw2/db2 accumulate (all NULL: input gradient only). */
int tg_d_head_fwd(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* l1, float* logit, float* prob,
                  int32_t B, int32_t T, int32_t H, void* stream);
int tg_d_head_bwd(const float* d_logit, const float* y, const float* l1, const float* w1, const float* w2, float* dy, float* dw1, float* db1,
                  float* dw2, float* db2, int32_t B, int32_t T, int32_t H, void* stream);

/* Head forward, per-clip GAN loss terms and head backward in ONE launch: what tg_d_head_fwd + (tg_gan_d_loss | the d_logit part of
 * tg_gan_g_loss) + tg_d_head_bwd compute in three.  y [n_rows][T][2H]; rows [0, n_real) are scored as real -- term = log(s + 1e-8),
 * d_logit = -scale_real s (1 - s) / (s + 1e-8) -- and rows [n_real, n_rows) as fake -- log(1 - s + 1e-8), +scale_fake s (1 - s) / (1 - s + 1e-8).
 * Discriminator step (train_gan.py:36-41): the stacked batch [real ; fake], n_rows = 2 n_real, both scales 1 / n_real, dis_error =
 * -sum(terms) / n_real.  Generator step (:55-57, 86-88): n_rows = n_real = B, scale_real = loss_gan_weight / B (0 in warm-up), no parameter
 * gradients, gen_error = -sum(terms) / B.  terms [n_rows]; out[0] = -sum(terms) / n_real summed by the last workgroup in the order of
 * tg_gan_d_loss, or out == NULL: the caller sums terms itself (saves the serial tail); counter (needed with out): one zero-initialised
 * device word the kernel leaves at zero (never shared by launches that may run concurrently).  dw1/db1/dw2/db2 accumulate (all NULL: none). */
int tg_d_head_step(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, float* l1, float* logit, float* prob,
                   float* d_logit, float* terms, float* out, uint32_t* counter, float* dy, float* dw1, float* db1, float* dw2, float* db2,
                   int32_t n_rows, int32_t n_real, float scale_real, float scale_fake, int32_t T, int32_t H, void* stream);

/* out[0] = mean |a - b| over n elements (F.l1_loss, train.py:282). */
int tg_l1_mean(const float* a, const float* b, int64_t n, float* out, void* stream);
/* y = 1 / (1 + exp(-x)) */
int tg_sigmoid(const float* x, float* y, int64_t n, void* stream);
/* dx = dy * y * (1 - y), y = sigmoid(x)  (torch.sigmoid backward, multimodal_context_net.py:250). */
int tg_sigmoid_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);

/* Cross-fade of consecutive synthesis windows (synthesize.py:145-153), in place on the new window:
 * next[b][j][:] = prev_tail[b][j][:] * (n-j)/(n+1) + next[b][j][:] * (j+1)/(n+1), j < n.  next: [B][T][D], prev_tail: [B][n][D]. */
int tg_window_blend(const float* prev_tail, float* next, int32_t B, int32_t T, int32_t D, int32_t n, void* stream);

/* Long-utterance synthesis on the device (csrc/utterance.hip; synthesize.py:82-119,162-207).  The window plan of utterance b occupies rows
 * [win_off[b], win_off[b+1]) of plan_win [G][4] = (audio_start, n_valid, spec_start, text length) and plan_text [G][text_stride]; it holds
 * integers only, computed once per utterance by the host.  win_idx [B] (device memory) is each row's window, clamped to the utterance's own
 * windows.  tg_window_stage writes out_audio [B][L] = audio[audio_off[b] + audio_start ...][0:n_valid] followed by zeros (null: no audio) and
 * out_text [B][text_w] = the first text_w entries of the window's plan_text row (null: no text); 16-byte copies where both sides are
 * aligned.  Bit-exact against the host path. */
int tg_window_stage(const float* audio, const int64_t* audio_off, const int32_t* win_off, const int32_t* win_idx, const int64_t* plan_win,
                    const int64_t* plan_text, int32_t text_stride, int32_t B, int32_t L, int32_t text_w, float* out_audio, int64_t* out_text,
                    void* stream);
/* The speech2gesture sibling: out [B][n_mels][width] = columns [spec_start, spec_start + width) of utterance b's spectrogram
 * [n_mels][(spec_off[b+1] - spec_off[b]) / n_mels] (offsets in elements), zeros past its last column.  Elements of elem_bytes = 2 (fp16) or 4
 * (fp32) bytes, copied as they are. */
int tg_spec_stage(const void* spec, const int64_t* spec_off, const int32_t* win_off, const int32_t* win_idx, const int64_t* plan_win, int32_t B,
                  int32_t n_mels, int32_t width, int32_t elem_bytes, void* out, void* stream);
/* In place on the stacked windows total [B][F][D] (row b holds n_win[b] * (n_poses - n_pre) + n_pre frames; n_win [B] int32 on the device,
 * all <= max_win), in this order, each part optional:
 *   smooth != 0        seq2seq's cubic least-squares fit around every window start (frames [i stride, i stride + 3 n_pre), i < n_win[b]);
 *   fade_start != null  per row with fade_start[b] >= 0: frames from fade_start[b] + n_pre on are zeroed (to F), frames [fade_start[b],
 *                      fade_start[b] + 2 n_pre) are replaced by the weighted quadratic fit; frames past the row's length count as zeros
 *                      (F >= max_win * stride + 3 n_pre);
 *   joints != null     joints [B][joints_frames][10][3] fp64 = bone integration of total + mean (fp64 [27]; D == 27).
 * proj (fp64): the (3 n_pre)^2 cubic projection, then the (2 n_pre)^2 weighted quadratic one, row-major; products are
 * accumulated in fp64 and rounded once.  Envelope: 1 <= n_pre <= 8, D <= 64, n_poses - n_pre >= 3 n_pre; refused otherwise. */
int tg_utterance_finish(float* total, int64_t F, int32_t B, int32_t D, const int32_t* n_win, int32_t max_win, int32_t n_poses, int32_t n_pre,
                        int32_t smooth, const double* proj, const int32_t* fade_start, const double* mean, double* joints, int64_t joints_frames,
                        void* stream);

/* Streaming synthesis (csrc/stream.hip; synthesize.GestureStream): audio and words arrive in pieces.  A stream of B rows keeps, all in device
 * memory, ring [B][R] fp32 with written [B] int64 (samples pushed so far) and word_ring [B][W][3] int32 with n_words [B] int64 (records pushed
 * so far).  A record is (absolute window index, frame in the window, word id): integers the host computed, one per window a word falls in.
 * tg_stream_push appends chunk [B][n] (device memory, rows chunk_stride floats apart) at written[b] mod R -- the chunk may straddle the wrap
 * point -- and, with m_max > 0, row b's records recs[b][1 .. 1 + 3 recs[b][0]) (recs [B][rec_stride] int32, device; recs[b][0] <= m_max) at
 * n_words[b] mod W; it advances both counters.  words_live: the host's count of ring slots from the oldest record a window still needs to
 * the newest.  Envelope, checked before anything is launched: 1 <= B <= 4, n >= 1, A + n <= R <= 2^30 (A: samples of a window, so that a
 * window that was incomplete before the push is still whole after it), 1 <= W <= 1024, words_live + m_max <= W, rec_stride >= 1 + 3 m_max. */
int tg_stream_push(const float* chunk, int64_t chunk_stride, int32_t n, const int32_t* recs, int32_t rec_stride, int32_t m_max, int32_t words_live,
                   float* ring, int64_t* written, int32_t* word_ring, int64_t* n_words, int32_t B, int32_t R, int32_t A, int32_t W, void* stream);
/* The inputs of window w = win[0] (int32, device memory; S: stride in samples): out_audio [B][A] = ring[b][(w S + k) mod R] for
 * k < min(A, written[b] - w S), zeros behind (null: no audio); out_text [B][T] int64 = per frame the id of the LAST pushed record of window w
 * on that frame, else 0 (null: no text).  Copies: bit-exact.  Envelope: 1 <= B <= 4, S >= 1, 1 <= A <= 2^25, A + 1 <= R <= 2^30,
 * 1 <= W <= 1024, 1 <= T <= 1024. */
int tg_stream_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win, int32_t B,
                    int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio, int64_t* out_text, void* stream);
/* The Seq2Seq model's text of window w = win[0] (csrc/stream_seq.hip; synthesize.Seq2SeqGestureStream) from the same word ring:
 * out_text [B][Te] int64 = [sos, the ids of EVERY record of window w in push order, eos, 0 ...], out_len [B] int64 = count + 2.  One workgroup
 * per row, an order-preserving compaction without atomics; ids are copied bit for bit.  A row with more than Te - 2 records of the window is
 * the host's to refuse before the push; the kernel clamps the count so that no index leaves the row.  Envelope: 1 <= B <= 4,
 * 1 <= W <= 1024, 2 <= Te <= 128. */
int tg_stream_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, int32_t B, int32_t W, int32_t Te, int64_t sos,
                         int64_t eos, int64_t* out_text, int64_t* out_len, void* stream);

/* Stream pool (csrc/stream_pool.hip; synthesize.StreamPool): the B <= 4 rows of a stream state are independent sessions.  Each row has its own
 * window counter, win [B] int32, and a launch touches only the rows it is told to: a row that is skipped keeps every bit of its rings, its
 * counters and its output rows.  One workgroup (or grid column) per row, no atomics, nothing waits on another workgroup.
 * tg_pool_push is tg_stream_push with one chunk length per row, n0 .. n3 by value (n[b] >= 0, 0 for b >= B): row b appends chunk[b][0 .. n[b])
 * and its records; a row with n[b] == 0 and recs[b][0] == 0 is skipped.  words_live + m_max is the slot count of the fullest word ring after
 * the push, counted from the oldest record a window of that row still needs.  Envelope: 1 <= B <= 4, some n[b] >= 1 or m_max >= 1,
 * A + max n <= R <= 2^30, A < R, 1 <= W <= 1024, words_live + m_max <= W, chunk_stride >= max n, rec_stride >= 1 + 3 m_max. */
int tg_pool_push(const float* chunk, int64_t chunk_stride, int32_t n0, int32_t n1, int32_t n2, int32_t n3, const int32_t* recs, int32_t rec_stride,
                 int32_t m_max, int32_t words_live, float* ring, int64_t* written, int32_t* word_ring, int64_t* n_words, int32_t B, int32_t R,
                 int32_t A, int32_t W, void* stream);
/* tg_stream_stage per row: row b with active[b] != 0 (int32 [B], device memory) gets the inputs of ITS window win[b]; the out_audio /
 * out_text rows of the other rows are not written.  Envelope: tg_stream_stage's. */
int tg_pool_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                  const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio, int64_t* out_text,
                  void* stream);
/* The tail of a window as one launch, for every row with active[b] != 0: out[b] = res[b] ([B][T][D], contiguous); if win[b] > 0 its first n_pre
 * frames are cross-faded with tail[b] ([B][n_pre][D]) exactly as tg_window_blend does; tail[b] = out[b][T - n_pre ..]; the next window's seed --
 * seed_layout 0: pre_seq [B][T][D + 1] as tg_make_pre_seq writes it (the n_pre frames and the constraint bit, zeros elsewhere), seed_layout 1:
 * pre [B][n_pre][D] --; then win[b] += 1.  Inactive rows: nothing is written.  Envelope: 1 <= B <= 4, 1 <= n_pre <= 8, 1 <= D <= 64,
 * n_pre < T <= 1024. */
int tg_pool_handover(const float* res, float* out, float* tail, float* seed, int32_t seed_layout, int32_t* win, const int32_t* active, int32_t B,
                     int32_t T, int32_t D, int32_t n_pre, void* stream);

/* Stream pool of the Seq2Seq model (csrc/stream_pool_seq.hip; synthesize.Seq2SeqStreamPool): the same per-row state, one workgroup per row, no
 * atomics, nothing waits on another workgroup; a row with active[b] == 0 leaves before any barrier and keeps every bit of what it owns.
 * tg_pool_stage_text is tg_stream_stage_text per row: row b with active[b] != 0 gets [sos, every record of ITS window win[b] in push order, eos,
 * 0 ...] in out_text[b] and count + 2 in out_len[b] (the count clamped to Te - 2); the other rows of out_text / out_len are not written.
 * Envelope: tg_stream_stage_text's, active and win [B] int32 non-null. */
int tg_pool_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, const int32_t* active, int32_t B, int32_t W, int32_t Te,
                       int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len, void* stream);
/* tg_pool_handover for the seed layout pre [B][n_pre][D], with the Seq2Seq model's smoothing of the window it hands over: per active row
 * out[b] = res[b], cross-faded with tail[b] where win[b] > 0; then frames [0, 3 n_pre) of out[b] are replaced by their cubic least-squares
 * fit -- proj: the (3 n_pre)^2 fp64 projection tg_utterance_finish takes, applied in the same order, so the bits are those of
 * tg_utterance_finish(smooth) on that window --; tail[b] = out[b][T - n_pre ..], seed[b] = tail[b], win[b] += 1.  The segment must lie inside
 * the window's first T - n_pre frames: the tail is then raw decoder output, as the next window's cross-fade and seed need it.
 * Envelope: 1 <= B <= 4, 1 <= n_pre <= 8, 1 <= D <= 64, 3 n_pre <= T - n_pre, T <= 1024; refused otherwise, nothing is launched. */
int tg_pool_handover_smooth(const float* res, float* out, float* tail, float* seed, int32_t* win, const int32_t* active, const double* proj,
                            int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream);

/* Sample-rate conversion to 16 kHz (csrc/resample.hip; the counterpart of scripts/synthesize.py's librosa.load(..., sr=16000); added under
 * ABI 11 -- new symbols only).  Rational polyphase resampling by L / M, L = 16000 / g, M = input_sr / g, g = gcd(16000, input_sr), with the
 * caller's tap table taps [L][K] fp32 (K even):  y[n] = sum_{k < K} x[(n M) div L - K/2 + 1 + k] * taps[(n M) mod L][k],  samples outside the
 * signal exact zeros, fp32 fused multiply-adds in increasing k.  A signal of n_in samples gives ceil(n_in L / M) outputs.
 * tg_resample: B signals packed in x, signal b = x[in_off[b] .. in_off[b+1]) -> y[out_off[b] ..), at most out_off[b+1] - out_off[b] samples
 * (in_off, out_off [B + 1] int64, device memory); max_out: the longest output, which sizes the grid.
 * Envelope: 1 <= B <= 65535, max_out >= 1, 1 <= L <= 640, M >= 1, K even in [2, 512]; refused otherwise, nothing is launched.  (A tile is
 * the largest power of two of outputs, at most 256, whose tap rows and input span fit the LDS: 256 at 48 kHz, 64 at 44.1 kHz.) */
int tg_resample(const float* x, const int64_t* in_off, const int64_t* out_off, int32_t B, int64_t max_out, const float* taps, int32_t L, int32_t M,
                int32_t K, float* y, void* stream);
/* The same conversion for 1 to 4 rows whose input arrives in chunks: row b appends chunk[b][0 .. n[b]) (n0 .. n3 by value, 0 for b >= B; rows
 * chunk_stride floats apart).  Per row, in device memory: carry [B][K - 1] (the last K - 1 input samples; zeros when the row is opened),
 * consumed [B] and produced [B] int64 (input samples taken, output samples written so far).  The call writes to out[b][0 ..) the outputs that
 * became final -- those whose whole tap span lies at or before the last input sample: produced becomes ((consumed - K/2) L - 1) div M + 1, or 0
 * while consumed <= K/2 -- and, for a row whose bit of flush_mask is set, everything up to ceil(consumed L / M) with zeros past the end of
 * the input.  Concatenated, a row's outputs are tg_resample's of the whole signal bit for bit.  A row with n[b] == 0 and no flush bit is not
 * touched.  The host mirrors both counters with the same integer expressions; nothing here is read back.
 * Envelope: 1 <= B <= 4, n[b] >= 0, some n[b] >= 1 or a flush bit, tg_resample's L, M, K, chunk_stride >= max n,
 * out_stride >= ceil((max n + (K/2 on a flush)) L / M) + 1. */
int tg_resample_stream(const float* chunk, int64_t chunk_stride, int32_t n0, int32_t n1, int32_t n2, int32_t n3, int32_t flush_mask, const float* taps,
                       int32_t L, int32_t M, int32_t K, float* carry, int64_t* consumed, int64_t* produced, float* out, int64_t out_stride, int32_t B,
                       void* stream);

/* Stream preview (csrc/stream_preview.hip; synthesize.GestureStream.preview / StreamPool.preview; added under ABI 11 -- new symbols only): the
 * window that is still filling, as the closing window of the utterance truncated now would run it, without touching the stream.  None of the
 * three stores to a ring, a counter, tail, a seed, win, active, the resampler's carry or the decoder's out.  One workgroup (or grid column)
 * per row, a row that is not selected leaves before any store, no atomics, nothing waits on another workgroup.
 * tg_resample_stream_peek: tg_resample_stream's flush of the rows in row_mask WITHOUT its stores to carry / consumed / produced: extra[b][0 ..)
 * (rows extra_stride floats apart) = the outputs from produced[b] up to ceil(consumed[b] L / M) out of [carry | zeros], the same tile body and
 * chain of fused multiply-adds, so the bits a flush would append.  The host knows the count: ceil(consumed L / M) - produced.
 * Envelope: 1 <= B <= 4, 1 <= row_mask < 2^B, tg_resample's L, M, K, extra_stride >= ceil((K/2) L / M) + 1. */
int tg_resample_stream_peek(int32_t row_mask, const float* taps, int32_t L, int32_t M, int32_t K, const float* carry, const int64_t* consumed,
                            const int64_t* produced, float* extra, int64_t extra_stride, int32_t B, void* stream);
/* tg_stream_stage / tg_pool_stage on rows that count as written[b] + extra_n[b] samples long: stream positions written[b] <= p < written[b] +
 * extra_n[b] read extra[b][p - written[b]] (rows extra_stride floats apart; e0 .. e3 by value, 0 for b >= B), zeros behind.  The window index
 * of row b is win[b] (int32 [B], device memory) or, win == null, w_value for every row; active (int32 [B]) may be null: every row.  With
 * every extra_n 0 the outputs are tg_stream_stage's / tg_pool_stage's bit for bit (one row body, stream_rows.hpp).  Writes out_audio and
 * out_text only.  Envelope: tg_stream_stage's, extra_n[b] >= 0, extra_stride >= max extra_n, extra and out_audio non-null if any extra_n > 0. */
int tg_stream_stage_preview(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                            int32_t w_value, const int32_t* active, const float* extra, int64_t extra_stride, int32_t e0, int32_t e1, int32_t e2,
                            int32_t e3, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio, int64_t* out_text,
                            void* stream);
/* tg_pool_handover's first half and nothing else: for every row with active[b] != 0 (active == null: every row) preview_out[b] = res[b]
 * ([B][T][D], contiguous), its first n_pre frames cross-faded with tail[b] exactly as tg_window_blend does where the row's window index --
 * win[b], or w_value if win == null -- is > 0.  tail, the seeds and win are not written; the preview_out rows of the other rows neither.
 * Envelope: tg_pool_handover's (1 <= B <= 4, 1 <= n_pre <= 8, 1 <= D <= 64, n_pre < T <= 1024). */
int tg_preview_handover(const float* res, const float* tail, const int32_t* win, int32_t w_value, const int32_t* active, int32_t B, int32_t T,
                        int32_t D, int32_t n_pre, float* preview_out, void* stream);

/* Synthesis queue (csrc/queue.hip; synthesize.generate_gestures_queue; added under ABI 11 -- new symbols only): N utterances on the R rows of
 * one window decoder.  sched [rounds][R][2] int32 (device memory) = (utterance, window) of every row in every round, (-1, -1) where the row
 * idles; rnd [R] int32 (device memory) counts each row's rounds, and row b reads its entry sched[rnd[b]][b]: no round number is passed, the
 * launches of every round are the same.  The plan tables are tg_window_stage's, of all N utterances (win_off [N + 1], plan_win [G][4],
 * plan_text [G][text_stride], audio_off [N + 1]).  One workgroup (or grid column) per row, plain loads and stores, no atomics, nothing waits
 * on another workgroup; an idle row -- an entry that names no window of an utterance, or rnd[b] outside [0, rounds) -- leaves before any
 * store.  The host guarantees that no two rows of a round run the same utterance.
 * tg_queue_stage, for row b running (u, i), with g = win_off[u] + i: out_audio[b] [L] = tg_window_stage's slice of utterance u (null: no
 * audio); out_text[b] [text_w] int64 = the first min(text_w, text_stride) ids of plan_text[g], zeros behind (null: no text) -- with out_len
 * non-null (the Seq2Seq model, 2 <= text_w = Te <= 128) the list's plan_win[g][3] ids, zeros behind, and out_len[b] = that length --;
 * vid[b] = vids[u] (int64; both null or neither); draw[b] [draw_w] = draws[g] (draws [G][draw_w], draw_w 16 or 32; both null or neither); and
 * where i == 0 the row's seed buffer (null: none) = utterance u's seed: seed_layout 0: pre_seq [R][T][D + 1], the n_pre frames of
 * seeds[u] ([N][n_pre][D]) with the constraint bit, zeros elsewhere; seed_layout 1: pre [R][n_pre][D] = seeds[u].  seeds == null, or
 * seed_on[u] == 0 (int32 [N]; null: every utterance has a seed): all zeros, no constraint bit.  Copies are bit-exact.
 * tg_queue_handover, for row b running (u, i): total[u][i (T - n_pre) .. + T) = res[b] ([R][T][D]), its first n_pre frames cross-faded with
 * tail[b] exactly as tg_window_blend does where i > 0 (total: [N][F][D]); tail[b] = the window's last n_pre frames; the next window's seed in
 * tg_pool_handover's seed_layout; then rnd[b] += 1.  An idle row with rnd[b] in [0, rounds) only has its counter advanced.
 * Envelope of both: rounds >= 1, 1 <= R <= 128, N >= 1, 1 <= n_pre <= 8, 1 <= D <= 64, n_pre < T <= 1024 (F >= T); refused otherwise,
 * nothing is launched. */
int tg_queue_stage(const int32_t* sched, const int32_t* rnd, int32_t rounds, int32_t R, int32_t N, const float* audio, const int64_t* audio_off,
                   const int32_t* win_off, const int64_t* plan_win, const int64_t* plan_text, int32_t text_stride, int32_t L, int32_t text_w,
                   float* out_audio, int64_t* out_text, int64_t* out_len, const int64_t* vids, int64_t* vid, const float* draws, float* draw,
                   int32_t draw_w, const float* seeds, const int32_t* seed_on, float* seed, int32_t seed_layout, int32_t T, int32_t D, int32_t n_pre,
                   void* stream);
int tg_queue_handover(const float* res, float* total, int64_t F, float* tail, float* seed, int32_t seed_layout, const int32_t* sched, int32_t* rnd,
                      int32_t rounds, const int32_t* win_off, int32_t R, int32_t N, int32_t T, int32_t D, int32_t n_pre, void* stream);

/* Wide stream pool (csrc/stream_pool_wide.hip: the push; csrc/stream_pool.hip: stage and hand-over, tg_pool_*'s kernels and launchers with
 * another row limit; synthesize.WideStreamPool; added under ABI 11 -- new symbols only): the stream pool's three
 * launches for 1 <= B <= 128 rows, with everything per row in device memory.  The state, the row bodies and every other bound are
 * tg_pool_*'s; for B <= 4 each entry writes what its tg_pool_* counterpart writes, bit for bit.  One workgroup (or grid column) per row, plain
 * loads and stores, no atomics, nothing waits on another workgroup; a row that is not selected leaves before any store and before any
 * barrier and keeps every bit it owns.
 * tg_wide_pool_push: the push as slices of one packed device buffer.  hdr [B][4] int32 = per row (n samples, sample offset, record count,
 * record offset); samples [samples_len] fp32 = the rows' chunks concatenated, no padding; recs [recs_len][3] int32 = the rows' records
 * (window, frame, word id) concatenated.  Row b appends samples[off_b .. off_b + n_b) to its ring and recs[roff_b .. roff_b + m_b) to its word
 * ring exactly as tg_pool_push's row does; a row with n_b == 0 and m_b == 0 is skipped.  n_max / m_max: the largest n_b / m_b (they size
 * nothing but the envelope check); words_live as for tg_pool_push.  The host validates the header before it uploads it; the kernel clamps
 * n_b to [0, n_max], m_b to [0, m_max] and both slices into samples / recs, so that no index leaves them.
 * Envelope: 1 <= B <= 128, n_max >= 0, m_max >= 0, n_max >= 1 or m_max >= 1, A + n_max <= R <= 2^30, A < R, 1 <= W <= 1024,
 * words_live + m_max <= W, n_max <= samples_len <= B n_max, m_max <= recs_len <= B m_max; samples (recs) may be null if n_max (m_max) is 0. */
int tg_wide_pool_push(const int32_t* hdr, const float* samples, int64_t samples_len, const int32_t* recs, int64_t recs_len, int32_t n_max,
                      int32_t m_max, int32_t words_live, float* ring, int64_t* written, int32_t* word_ring, int64_t* n_words, int32_t B, int32_t R,
                      int32_t A, int32_t W, void* stream);
/* tg_pool_stage for 1 <= B <= 128: row b with active[b] != 0 gets the inputs of ITS window win[b] (win, active: int32 [B], device memory); the
 * out_audio / out_text rows of the other rows are not written.  Envelope: tg_pool_stage's with 1 <= B <= 128. */
int tg_wide_pool_stage(const float* ring, const int64_t* written, const int32_t* word_ring, const int64_t* n_words, const int32_t* win,
                       const int32_t* active, int32_t B, int32_t R, int32_t S, int32_t A, int32_t W, int32_t T, float* out_audio, int64_t* out_text,
                       void* stream);
/* tg_pool_handover for 1 <= B <= 128, both seed layouts (0: pre_seq [B][T][D + 1], 1: pre [B][n_pre][D]).  Envelope: tg_pool_handover's with
 * 1 <= B <= 128. */
int tg_wide_pool_handover(const float* res, float* out, float* tail, float* seed, int32_t seed_layout, int32_t* win, const int32_t* active,
                          int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream);
/* Wide stream pool at any sample rate (csrc/stream_pool_wide_rs.hip; synthesize.WideResampledStreamPool; added under ABI 11 -- new symbols
 * only): tg_resample_stream and tg_wide_pool_push as ONE launch for 1 <= B <= 128 rows, one workgroup per row.  hdr, samples and recs are
 * tg_wide_pool_push's packed pieces, with n_b counting INPUT-rate samples; taps [L][K], carry [B][K - 1], consumed [B] and produced [B] are
 * tg_resample_stream's, ring, written, word_ring and n_words tg_pool_push's.  Row b takes samples[off_b .. off_b + n_b) into its resampler
 * row; the outputs that became final -- n_new = ((consumed - K/2) L - 1) div M + 1 - produced, or, for the one row b == flush_row whose input
 * has ended, ceil(consumed L / M) - produced with zeros past the end -- go to its ring at (written[b] + r) mod R, bit for bit the samples
 * tg_resample gives for the whole signal; the carry is rewritten, the row's m_b records are appended to its word ring, and consumed,
 * produced, written (+ n_new) and n_words (+ m_b) advance.  A row with n_b == 0, m_b == 0 that is not flush_row is not touched; a row with
 * records only keeps its resampler row.  flush_row: -1, or the row to flush.  The host mirrors every counter with the same integer
 * expressions; nothing is read back.  For B <= 4 the call writes what tg_resample_stream followed by tg_pool_push write.  The kernel clamps
 * the header as tg_wide_pool_push's does and n_new to [0, ceil((n_max + (K/2 on a flush)) L / M) + 1].
 * Envelope: 1 <= B <= 128, -1 <= flush_row < B, tg_resample's L, M, K, n_max >= 0, m_max >= 0, n_max >= 1 or m_max >= 1 or flush_row >= 0,
 * A >= 1, A + ceil((n_max + (K/2 on a flush)) L / M) + 1 <= R <= 2^30, 1 <= W <= 1024, words_live + m_max <= W, n_max <= samples_len <=
 * B n_max, m_max <= recs_len <= B m_max; samples (recs) may be null if n_max (m_max) is 0; refused otherwise, nothing is launched. */
int tg_wide_pool_push_resampled(const int32_t* hdr, const float* samples, int64_t samples_len, const int32_t* recs, int64_t recs_len, int32_t n_max,
                                int32_t m_max, int32_t words_live, int32_t flush_row, const float* taps, int32_t L, int32_t M, int32_t K,
                                float* carry, int64_t* consumed, int64_t* produced, float* ring, int64_t* written, int32_t* word_ring,
                                int64_t* n_words, int32_t B, int32_t R, int32_t A, int32_t W, void* stream);

/* Wide stream pool of the Seq2Seq model (csrc/stream_pool_wide_seq.hip: the push; csrc/stream_pool_seq.hip: text staging and hand-over,
 * tg_pool_stage_text's and tg_pool_handover_smooth's kernels and launchers with another row limit; synthesize.WideSeq2SeqStreamPool; added under
 * ABI 11 -- new symbols only): the Seq2Seq stream pool's three launches for 1 <= B <= 128 rows.  One workgroup per row, plain loads and
 * stores, no atomics, nothing waits on another workgroup; a row that is not selected leaves before any store and before any barrier and
 * keeps every bit it owns.  For B <= 4 the stage and the hand-over write what their tg_pool_* counterparts write, bit for bit.
 * tg_wide_pool_push_words: the tick of a model that reads no sample.  hdr [B][4] int32 = per row (n samples, unused, record count, record
 * offset) -- tg_wide_pool_push's header --; recs [recs_len][3] int32 = the rows' records (window, frame, word id) concatenated.  Row b appends
 * recs[roff_b .. roff_b + m_b) to its word ring exactly as tg_wide_pool_push's row does and adds n_b to written[b] (n_words[b] += m_b); there
 * is no sample ring and no sample is copied.  A row with n_b == 0 and m_b == 0 is skipped.  The kernel clamps n_b to >= 0, m_b to [0, m_max]
 * and the slice into recs, so that no index leaves it.  words_live as for tg_pool_push.
 * Envelope: 1 <= B <= 128, m_max >= 0, 1 <= W <= 1024, words_live >= 0, words_live + m_max <= W, m_max <= recs_len <= B m_max; recs may be null
 * if m_max is 0; refused otherwise, nothing is launched. */
int tg_wide_pool_push_words(const int32_t* hdr, const int32_t* recs, int64_t recs_len, int32_t m_max, int32_t words_live, int64_t* written,
                            int32_t* word_ring, int64_t* n_words, int32_t B, int32_t W, void* stream);
/* tg_pool_stage_text for 1 <= B <= 128.  Envelope: tg_pool_stage_text's with 1 <= B <= 128. */
int tg_wide_pool_stage_text(const int32_t* word_ring, const int64_t* n_words, const int32_t* win, const int32_t* active, int32_t B, int32_t W,
                            int32_t Te, int64_t sos, int64_t eos, int64_t* out_text, int64_t* out_len, void* stream);
/* tg_pool_handover_smooth for 1 <= B <= 128.  Envelope: tg_pool_handover_smooth's with 1 <= B <= 128. */
int tg_wide_pool_handover_smooth(const float* res, float* out, float* tail, float* seed, int32_t* win, const int32_t* active, const double* proj,
                                 int32_t B, int32_t T, int32_t D, int32_t n_pre, void* stream);

/* evaluate_testset metrics of one batch (train.py:282-310; utils/data_utils.py:77-98): out/target direction vectors [B][T][27],
 * mean_dir_vec [27].  sums[0] = sum |joint error| over frames >= n_pre and 10x3 joints, sums[1] = sum |second-difference error| over
 * T-2 frames, sums[2] = sum |out - target|.  (joint_mae = sums[0]/(B*(T-n_pre)*30), accel = sums[1]/(B*(T-2)*30), l1 = sums[2]/(B*T*27).) */
int tg_pose_metrics(const float* out_dir_vec, const float* target_dir_vec, const float* mean_dir_vec, int32_t B, int32_t T,
                    int32_t n_pre, double* sums, void* stream);

/* FGD autoencoder loss (train_feature_extractor.py:64-72): loss = sum_b [mean|r-t| + mean|dr-dt|];
 * out[0] = loss, d_recon = d loss / d recon. */
int tg_ae_loss(const float* recon, const float* target, int32_t B, int32_t T, int32_t D, float* out, float* d_recon,
               void* stream);

/* One FGD autoencoder training step up to the gradients (scripts/train_feature_extractor.py:54-97 on model/embedding_net.py:42-82,165-217:
 * PoseEncoderConv + PoseDecoderConv, 34 frames x 27, variational_encoding = False) in 18 launches (ABI 5; csrc/ae_step.hip): forward in
 * train mode (the eight BatchNorms' running statistics advance), loss = sum_b [mean |recon - x| + mean |d recon - d x|], and every parameter
 * gradient WRITTEN (not accumulated) into `grads` at the parameter's offset; fc_logvar receives no gradient (:58) and is not touched.
 * With adam_m / adam_v (the optimiser's moment slabs) the last launch also applies torch.optim.Adam(lr, betas, eps) to every parameter it has a
 * gradient for -- the step is then complete (fc_logvar is skipped like a parameter whose .grad is None); without them tg_adam_step over the slab
 * completes it.  *step (device Adam counter, may be NULL) is advanced by one by the first launch.
 * off[44]: offsets in floats (multiples of 4) of, in this order: pose_encoder.net.{0,1,2}: {0.weight, 0.bias, 1.weight, 1.bias} each; net.3.{weight,
 * bias}; out_net.0.{weight, bias}, out_net.1.{weight, bias}, out_net.3.{..}, out_net.4.{..}, out_net.6.{..}; fc_mu.{..}; decoder.pre_net.0.{..},
 * pre_net.1.{..}, pre_net.3.{..}; decoder.net.0.{..}, net.1.{..}, net.3.{..}, net.4.{..}, net.6.{..}, net.7.{..}.
 * running_mean / running_var / num_batches_tracked[8]: the BatchNorms in forward order (encoder net.0-2, out_net.1, out_net.4, pre_net.1, decoder
 * net.1, net.4); a NULL pair skips that update.  ws: tg_ae_step_ws_bytes(B) bytes, 16-byte aligned, ZERO before the first use; a complete step
 * leaves its statistics block zero again (after an aborted step: zero it).  recon [B][34][27] and feat [B][32] (= mu) are optional outputs.
 * last_phase: 0 = the whole step; 1..18 = stop after that launch (tests).  2 <= B <= 256 (tg_ae_step_supported). */
typedef struct {
    const float* x;                       /* [B][34][27] */
    float* params;
    float* grads;
    int32_t off[44];
    float* running_mean[8];
    float* running_var[8];
    int64_t* num_batches_tracked[8];
    void* ws;
    int64_t ws_bytes;
    float* loss;                          /* [1] */
    float* recon;
    float* feat;
    int32_t* step;
    int32_t B;
    float bn_eps, momentum;
    int32_t last_phase;
    float* adam_m;                        /* Adam moments, slab images like params (both or neither) */
    float* adam_v;
    float lr, beta1, beta2, adam_eps;
} tg_ae_step_args;
int32_t tg_ae_step_supported(int32_t B);
int64_t tg_ae_step_ws_bytes(int32_t B);
int tg_ae_train_step(const tg_ae_step_args* args, void* stream);

/* ---- optimiser (torch.optim.Adam, train.py:104-109): one fused launch over a flat parameter slab ------
 * step_dev: device int32 step counter, incremented by tg_counter_inc BEFORE the update (graph-replay safe). */
int tg_counter_inc(int32_t* counter, void* stream);
int tg_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                 float eps, const int32_t* step_dev, void* stream);

/* ---- Speech2Gesture baseline (ABI 9; model/speech2gesture.py, train_eval/train_speech2gesture.py) ------------------------------------------
 * 2-D convolution as an implicit GEMM (csrc/conv2d.hip): activations channel-last (B, H, W, C) fp32 -- x may be fp16 (x_half = 1: the
 * spectrogram as the loader delivers it) in the forward and weight-gradient calls --, weights in nn.Conv2d's layout [Co][Ci][kh][kw].
 * Geometry: output Ho x Wo, stride 1 or 2 in both axes, explicit top / left zero padding (pad_top < kh, pad_left < kw); bottom / right zeros
 * come from the bounds, so TF "SAME" (the odd extra zero bottom / right) is pad_top = total / 2 with Ho = ceil(H / stride).  bf16 x 3
 * operand split, fp32-accurate; math mode 1: plain bf16 operands. */
/* y (B, Ho, Wo, Co) = conv(x) + bias (bias may be NULL). */
int tg_conv2d_fwd(const void* x, int32_t x_half, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W, int32_t Ci,
                  int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* stream);
/* dx (B, H, W, Ci) (+)= input gradient of dy (B, Ho, Wo, Co). */
int tg_conv2d_dgrad(const float* dy, const float* w, float* dx, int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co,
                    int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* stream);
/* workspace of tg_conv2d_wgrad for this geometry, in bytes (*bytes). */
int tg_conv2d_wgrad_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top,
                             int32_t pad_left, int32_t Ho, int32_t Wo, int64_t* bytes);
/* dw [Co][Ci][kh][kw] (+)= weight gradient: split-K partials in ws, combined in a fixed order in fp64 (bitwise repeatable in every mode).
 * The bias gradient is tg_colsum over dy. */
int tg_conv2d_wgrad(const float* dy, const void* x, int32_t x_half, float* dw, int32_t accumulate, float* ws, int64_t ws_bytes, int32_t B,
                    int32_t H, int32_t W, int32_t Ci, int32_t Co, int32_t kh, int32_t kw, int32_t stride, int32_t pad_top, int32_t pad_left,
                    int32_t Ho, int32_t Wo, void* stream);
/* make_1d: Upsample((Hout, 1), bilinear, align_corners=False) of x (B, Hin, Win, C) where only column `col` contributes (weight 1):
 * y (B, Hout, C), rows by torch's half-pixel rule clamped at the edges.  The backward WRITES dx (B, Hin, Win, C), zeros off column col. */
int tg_s2g_rows_interp(const float* x, float* y, int32_t B, int32_t Hin, int32_t Win, int32_t col, int32_t C, int32_t Hout, void* stream);
int tg_s2g_rows_interp_bwd(const float* dy, float* dx, int32_t B, int32_t Hin, int32_t Win, int32_t col, int32_t C, int32_t Hout, void* stream);
/* UnetUp: y[b, t] = x[b, t / 2] + skip[b, t], t < Ls <= 2 Lx (repeat_interleave x 2, crop, add); backward dx[b, l] (+)= dy[b, 2l] + dy[b, 2l + 1]
 * (the skip's gradient is dy itself). */
int tg_s2g_up_add(const float* x, const float* skip, float* y, int32_t B, int32_t Lx, int32_t Ls, int32_t C, void* stream);
int tg_s2g_up_add_bwd(const float* dy, float* dx, int32_t B, int32_t Lx, int32_t Ls, int32_t C, int32_t accumulate, void* stream);
/* first difference over time: y[b, t] = x[b, t + 1] - x[b, t] (B, T - 1, C); backward dx (B, T, C) (+)=. */
int tg_s2g_diff(const float* x, float* y, int32_t B, int32_t T, int32_t C, void* stream);
int tg_s2g_diff_bwd(const float* dy, float* dx, int32_t B, int32_t T, int32_t C, int32_t accumulate, void* stream);
/* LSGAN term: loss[0] = mean((x - target)^2) over n values (one workgroup, fp64 sums in a fixed order); dx (may be NULL) = scale 2 (x - target) / n. */
int tg_s2g_mse_const(const float* x, int64_t n, float target, float scale, float* loss, float* dx, void* stream);
/* gradient of mean |a - b| (tg_l1_mean): d = sign(a - b) / n. */
int tg_s2g_l1_grad(const float* a, const float* b, float* d, int64_t n, void* stream);

/* ---- log-mel spectrogram (ABI 10; utils/data_utils.py:34-38 extract_melspectrogram: librosa.feature.melspectrogram(n_fft = 1024, hop_length = 512,
 * power = 2) with 128 Slaney mels over 0 .. 8 kHz, power_to_db(ref = np.max), the fp16 cast) for N clips of L samples at 16 kHz in two launches
 * (csrc/logmel.hip).  Frames: center = True, F = 1 + L / 512, frame t = samples 512 t - 512 .. 512 t + 511 of the clip, the boundary read by index
 * arithmetic -- pad_mode 0: reflected (L >= 513), 1: zeros.  Periodic Hann window, |rfft|^2 over 513 bins, mel filters gathered in bin order,
 * db = 10 log10(max(M, 1e-10)) - 10 log10(max(max M, 1e-10)) with the maximum over the whole clip, floored at -80.  No atomics: bitwise repeatable.
 * tg_logmel_query: sizes[0] = F, sizes[1] = floats of the constant table, sizes[2] = bytes of workspace for (N, L).
 * tables (device, sizes[1] floats, built by the caller in fp64 and rounded once): [0, 1024) exp(-2 pi i k / 1024), k < 512, as (re, im) pairs;
 * [1024, 2048) the window; [2048, 5120) filter weights [24][128] (weight j of filter i at j * 128 + i, zero past the filter's last bin);
 * [5120, 5248) every filter's first bin as a float.  audio: clip n at audio + n * audio_stride.  out: (N, 128, F), fp32 or (out_half = 1) fp16 = the
 * round-to-nearest-even cast of the fp32 result.  ws: sizes[2] bytes of scratch, no initialisation needed. */
int tg_logmel_query(int32_t N, int32_t L, int64_t* sizes);
int tg_logmel(const float* audio, int64_t audio_stride, int32_t N, int32_t L, int32_t pad_mode, const float* tables, int64_t table_floats, void* ws,
              int64_t ws_bytes, void* out, int32_t out_half, void* stream);

/* ---- training samples from raw clips (ABI 11; data_loader/data_preprocessor.py:66-170, data_loader/motion_preprocessor.py:32-87,
 * utils/data_utils.py:46-56, data_loader/calculate_motion_stats.py:33-44; csrc/preprocess.hip).  A BATCH is many clips packed into one device buffer
 * and described by device-resident tables of 8-byte words (the host builds them and ships them with one copy per batch); one call covers the whole
 * batch.  Skeleton frames are 30 values (10 joints x 3), fp32 or (half = 1) fp16.  Doubles travel in the tables, never as arguments.  No atomics,
 * fixed reduction orders, fp64 accumulators: bitwise repeatable.  The host cannot inspect the tables, so the kernels check every table entry against
 * the extents given here and skip an entry that points outside (nothing is read or written there).
 *
 * tg_pose_resample -- resample_pose_seq (data_utils.py:46-56).  clips: n_clips records {int64 src_row0, int64 n, int64 dst_row0, int64 m, double step},
 * in increasing dst_row0: clip c owns frames src_row0 .. src_row0 + n - 1 of src (src_rows frames) and writes m = len(np.arange(0, n, step)) frames from
 * dst_row0 on (dst_rows frames in all), step = n / (duration * fps).  Output frame k is interp1d(kind = 'linear', fill_value = 'extrapolate') at
 * x = k * step, formed in fp64: segment hi = clip(ceil(x), 1, n - 1), lo = hi - 1, y = (y[hi] - y[lo]) * (x - lo) + y[lo] with the difference taken
 * in the input dtype (as numpy subtracts the arrays) and everything after it in fp64; x > n - 1 (an up-sampled clip) extrapolates along the last
 * segment.  The result is rounded once to the input dtype.  n = 1 copies the frame.
 *
 * tg_clip_windows -- window w = frames win_row0[w] .. + n_poses - 1 of skel (int64 table; the host adds the clip's first row and start_idx).
 * consts: 61 doubles = mean_pose[30], mean_dir_vec[27], thresholds {0.02, 30, 20, 0.0014} (pose difference, max / mean spine angle in degrees,
 * wrist variance).  Outputs: poses (n_windows, n_poses, 30) in the input dtype, the slice; vec (n_windows, n_poses, 27) fp32 = the nine unit vectors
 * of dir_vec_pairs (a zero-length bone gives zeros, sklearn.preprocessing.normalize) minus mean_dir_vec, formed in fp64 and rounded once;
 * stats (n_windows, 6) fp32 = mean |x - mean_pose|, max and mean over frames of arccos(clip(u . (0, -1, 0), -1, 1)) in degrees with u the unit vector
 * joint 1 - joint 0, the summed population variance of joint 6 and of joint 9 over the window, the count of non-finite inputs;
 * verdict (n_windows) int32 = 0 PASS, 1 "pose" (stats[0] < th0), 2 "spine angle" (stats[1] > th1 or stats[2] > th2), 3 "motion" (both variances < th3),
 * the first failing check in that order, decided on the fp64 values; -1: the table entry lies outside skel.
 *
 * tg_clip_slices -- window w copies `len` elements per row of a signal of `rows` rows: table records {int64 base, int64 L, int64 row_stride,
 * int64 start} (element units; row r of the signal begins at src + base + r * row_stride and holds L elements).  Element j of row r is index
 * start + j, read past the end as np.pad(mode = 'symmetric') does: q = (start + j) mod 2 L, q >= L -> 2 L - 1 - q (any padding length).  dst
 * (n_windows, rows, len).  elem_bytes 4 serves raw audio (rows = 1), 2 the fp16 spectrogram (rows = 128, slices along time).  Bit-exact.
 *
 * tg_motion_stats -- calculate_data_mean (calculate_motion_stats.py:33-44) over n_rows frames: out[0..30) the mean pose, [30, 57) the mean unit bone
 * vector, [57, 66) the mean bone length, doubles; fp64 partial sums per workgroup in ws (tg_motion_stats_query: sizes[0] = workgroups,
 * sizes[1] = bytes of ws), added in workgroup order by a second launch.  Batches are combined by the caller, weighted by their frame counts. */
int tg_pose_resample(const void* src, int64_t src_rows, int32_t half, const void* clips, int64_t clip_bytes, int32_t n_clips, void* dst,
                     int64_t dst_rows, void* stream);
int tg_clip_windows(const void* skel, int64_t skel_rows, int32_t half, const void* win_row0, int64_t table_bytes, int32_t n_windows, int32_t n_poses,
                    const void* consts, int64_t const_bytes, void* poses, float* vec, float* stats, int32_t* verdict, void* stream);
int tg_clip_slices(const void* src, int64_t src_elems, int32_t elem_bytes, int32_t rows, const void* table, int64_t table_bytes, int32_t n_windows,
                   int32_t len, void* dst, void* stream);
int tg_motion_stats_query(int64_t n_rows, int64_t* sizes);
int tg_motion_stats(const void* skel, int64_t n_rows, int32_t half, void* ws, int64_t ws_bytes, void* out, void* stream);

/* ---- autoencoder batches from raw Human3.6M positions (added under ABI 11; data_loader/h36m_loader.py:16-17, :37-42, :44-64, :69-106,
 * utils/data_utils.py:77-120; csrc/h36m.hip).  The conventions of the block above: actions packed into one device buffer, windows described by a
 * device-resident int64 table, one call per stage and batch, fp64 per-thread arithmetic without fused multiply-adds, no atomics, bitwise repeatable;
 * every table entry is checked against the extents given here, an entry that points outside is skipped and flagged.
 *
 * tg_h36m_normalize -- Human36M.normalize per frame.  positions: (rows, n_joints, 3) fp32, n_joints >= 28 (32 in data_3d_h36m.npz); out: (rows, 30)
 * fp32, the packed skeleton format of the block above, row r from frame r.  Per frame: the twelve target_joints {1, 6, 12, 13, 14, 15, 17, 18, 19, 25,
 * 26, 27} are gathered; gathered joint 2 is subtracted from all twelve in fp32; (x, y, z) becomes (x, -z, y) (:73-75); with hip = joint 1 - joint 0
 * (fp32), angle = pi - atan2(hip_z, hip_x) in fp64; deg = angle * (180 / pi); 0 < deg < 180 keeps the angle, 180 < deg < 360 subtracts
 * 360 * (pi / 180), anything else (exactly 0, 180 or 360 degrees) is left alone (:81-84, strict inequalities); with a = cos(angle / 2) and
 * c = -sin(angle / 2) the matrix of :93-106 about (0, 1, 0) is {{aa - cc, 0, -2 ac}, {0, aa + cc, 0}, {2 ac, 0, aa - cc}}; every joint becomes the
 * row vector joint @ matrix, the fp32 operands converted to fp64, the three products added left to right, the sum rounded once to fp32; joints 0 and 1
 * are dropped.
 *
 * tg_h36m_samples -- Human36M.__getitem__ for n_windows windows.  Window w is rows win_row0[w] + k * frame_stride, k < n_poses, of skel (skel_rows, 30)
 * (the reference: n_poses 34, frame_stride 2).  Per frame, in fp64: the nine bone differences of dir_vec_pairs, each taken in fp32 (numpy subtracts
 * the fp32 arrays); unit vectors d / sqrt(dx dx + dy dy + dz dz), a zero-length bone gives zeros; the joints rebuilt from the bone lengths {0.26, 0.18,
 * 0.14, 0.22, 0.36, 0.33, 0.22, 0.36, 0.33} with the root at the origin (parent + length * unit, multiply then add); the additive noise on all 30
 * coordinates, if any; the nine unit vectors again, now from fp64 differences; minus mean_dir_vec (27 doubles in device memory, mean_bytes >= 216).
 * Outputs: poses (n_windows, n_poses, 30) fp32 = the rebuilt (noisy) joints, vec (n_windows, n_poses, 27) fp32, each rounded once;
 * flag (n_windows) int32 = 0, or -1 where the window does not lie inside skel: nothing is read, poses and vec of that window are not written.
 * Noise: (a) noise == NULL and rng_state == NULL: none.  (b) noise: (n_windows, n_poses, 30) doubles (noise_bytes >= that), the final additive
 * values.  (c) rng_state (device uint64[2], see "randomness" above; never together with noise): drawn in the same launch, nothing stored -- the value
 * for window slot i (its index in win_row0) and coordinate e < n_poses * 30 is (double)z * (double)std_i, z being the float that
 * tg_normal(out, n, rng_state, noise_site) would write at index i * n_poses * 30 + e, and std_i = std_large where
 * tg_dropout_mask(mask, n, p_large, rng_state, select_site) would write 0 at index i (probability p_large), std_small otherwise.  Both draws are pure
 * functions of (state, site, index): they do not depend on the length n of the call they are compared with (any n > index, vectorised or not).
 * 0 <= p_large < 1 as for tg_dropout_mask.  The reference's values (:50-56): p_large 0.2, std_large sqrt(0.002), std_small sqrt(0.0001). */
int tg_h36m_normalize(const float* positions, int64_t rows, int32_t n_joints, float* out, void* stream);
int tg_h36m_samples(const float* skel, int64_t skel_rows, const void* win_row0, int64_t table_bytes, int32_t n_windows, int32_t n_poses,
                    int32_t frame_stride, const void* mean_dir_vec, int64_t mean_bytes, const void* noise, int64_t noise_bytes, const uint64_t* rng_state,
                    uint32_t noise_site, uint32_t select_site, float p_large, float std_large, float std_small, float* poses, float* vec, int32_t* flag,
                    void* stream);

/* ---- Frechet gesture distance on the device (added under ABI 11 -- new symbols only, nothing existing changes, so the version stays; model/embedding_space_evaluator.py:74-156; csrc/fgd.hip).  The score is evaluated
 * in the symmetric formulation Tr sqrt(S1 S2) = sum sqrt(eig(S1^1/2 S2 S1^1/2)) in fp64: always real and finite, so the reference's eps-offset retry
 * (:139-144) and its imaginary-component branch (:147-151) cannot occur; the means are fp64 where the reference's are fp32.
 *
 * State: one caller-owned buffer of tg_fgd_state_doubles(D) doubles per evaluator (1 <= D <= 32; the size comes back through *doubles, the return
 * value is the status like everywhere else).  Layout: [0] first-push flag, [1] pushes, [2] sum over pushes of (recon_err_fake - recon_err_real),
 * [3] sum over rows of sum_j |real - generated|, [4, 4 + D) the pivot K = the mean of the first pushed real batch (formed on the device inside that
 * push); then for the real set and for the generated set {n, sum (x - K) [D], sum (x - K)(x - K)^T [D][D]}; the rest is the push workspace.  The
 * pivot keeps features far from zero from cancelling in S - s s^T / n.  States whose pivots agree are additive.
 *
 * tg_fgd_reset -- zeroes the state (not the workspace).
 * tg_fgd_push  -- real_feat, gen_feat: (B, D) fp32 row-major, paired rows; recon_err_real / recon_err_fake: device fp32 scalars, either may be NULL
 *   (that term is then skipped).  fp64 accumulation; rows are spread over up to 16 workgroups of 256 rows each (more rows: they stride), partial
 *   sums go to the workspace and a second launch adds them to the state in workgroup order.  No floating-point atomics: two identical runs leave
 *   bit-identical states.  The inputs must not overlap the state.
 * tg_fgd_scores -- one workgroup.  mu and cov (ddof = 1) of both sets from the shifted sums, symmetrised; cyclic Jacobi (round-robin parallel
 *   ordering: the D / 2 disjoint rotations of a step together) on S1 = the generated set's covariance, R = S1^1/2 with negative eigenvalues clamped
 *   to 0; M = R S2 R symmetrised, Jacobi again for its eigenvalues l.  A solve stops when the off-diagonal Frobenius norm is <= 2^-52 ||A||_F, or
 *   after 30 sweeps.  out (TG_FGD_OUT_DOUBLES doubles, 11 used): [0] fgd = ||mu1 - mu2||^2 + tr S1 + tr S2 - 2 sum sqrt(max(l, 0)),
 *   [1] feat_dist = mean over rows of sum_j |real - generated|, [2] n (rows per set), [3] mean over pushes of (recon_err_fake - recon_err_real),
 *   [4] tr S1, [5] tr S2, [6] ||mu1 - mu2||^2, [7] sum sqrt l, [8] / [9] the sweeps of the two solves, [10] status: bit 0 a solve reached the sweep
 *   cap, bit 1 n < 2 (then [0] and [4 .. 9] are NaN).
 * tg_fgd_from_stats -- the same finish for given fp64 moments (mu [D], S [D][D] row-major, device memory): frechet_distance on the device; out[1],
 *   out[2], out[3] are 0. */
#define TG_FGD_OUT_DOUBLES 16
int tg_fgd_state_doubles(int32_t D, int64_t* doubles);
int tg_fgd_reset(void* state, int32_t D, void* stream);
int tg_fgd_push(void* state, const float* real_feat, const float* gen_feat, int32_t B, int32_t D, const float* recon_err_real,
                const float* recon_err_fake, void* stream);
int tg_fgd_scores(const void* state, int32_t D, double* out, void* stream);
int tg_fgd_from_stats(const double* mu1, const double* S1, const double* mu2, const double* S2, int32_t D, double* out, void* stream);

/* ---- General GRU recurrence (csrc/gru_seq.hip): nn.GRU semantics for ONE layer with D = 1 or 2 directions, per-row lengths, an initial state
 * and the final state -- what pack_padded_sequence -> nn.GRU -> pad_packed_sequence computes (seq2seq_net.py:51-56), and a GRU started from
 * a given hidden state (seq2seq_net.py:181, embedding_net.py:251-253).  One launch per time step; no workgroup waits on another.
 *   gi      [D][B][T][3H]  input projections with b_ih added; gi[:, b, t] at t >= lengths[b] is never read
 *   w_hh_*  [3H][H], b_hh_* [3H] per direction (the _rev pair is ignored, and may be NULL, at D = 1)
 *   h0      [D][B][H] or NULL (zeros)
 *   lengths [B] int64 in DEVICE memory or NULL (every row has T steps); valid entries are 1 .. T in any order.  An entry outside that range
 *           skips the row (y = 0, h_n = h0, dgi = dgh = 0, dh0 = dh_n) and sets *flag = 1 (flag: one int32 word zeroed by the caller, or
 *           NULL); nothing outside the row's own positions is read or written.
 *   y       [B][T][D*H]    direction d in columns [d*H, (d+1)*H); EXACTLY 0 at t >= lengths[b].  The forward direction runs t = 0 .. len-1, the
 *           reverse direction STARTS at t = len-1 and runs down to 0.
 *   h_n     [D][B][H]      the last state of each direction: y[b, len-1, :H] and y[b, 0, H:], bit for bit
 *   save    [D][B][T][5H]  the tape r, z, n, W_hn h + b_hn, h_prev (h_prev: the state the step started from, h0 at a row's first step), zeros
 *           at t >= lengths[b]; NULL for a forward without a backward.  dW_hh = dgh^T @ save[..., 4H:5H].
 * Backward: dy [B][T][D*H] (never read at t >= lengths[b]), dh_n [D][B][H] or NULL, w_hh_t_* the TRANSPOSED recurrent weights [H][3H];
 * dgi, dgh [D][B][T][3H] as tg_gru_backward gives them, EXACTLY 0 at t >= lengths[b]; dh0 [D][B][H] or NULL (not wanted);
 * dh_scratch: 2*D*B*H floats.
 * Envelope: D in {1, 2}, B >= 1, T >= 1, H % 4 == 0, 8 <= H <= 320 (and ceil(B/32) * ceil(H/16) * D workgroups fit an int32).  Outside it
 * the entries return non-zero, set tg_last_error and launch nothing; tg_gru_seq_supported writes 1 / 0 for a shape of positive sizes. */
int tg_gru_seq_supported(int32_t B, int32_t T, int32_t H, int32_t D, int32_t* supported);
int tg_gru_seq_forward(const float* gi, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev,
                       const float* h0, const void* lengths, float* y, float* h_n, float* save, int32_t* flag, int32_t B, int32_t T,
                       int32_t H, int32_t D, void* stream);
int tg_gru_seq_backward(const float* dy, const float* dh_n, const float* save, const float* w_hh_t_fwd, const float* w_hh_t_rev,
                        const void* lengths, float* dgi, float* dgh, float* dh0, float* dh_scratch, int32_t B, int32_t T, int32_t H,
                        int32_t D, void* stream);

/* ---- Bahdanau attention of the Seq2Seq decoder, one decoder step per launch (csrc/attn.hip; model/seq2seq_net.py:59-89, 165-167):
 *   e[b,t,:] = tanh(q[b] + keys[b,t,:]), s[b,t] = v . e[b,t,:], w[b,:] = softmax_t(s[b,:]) over ALL Te positions (no padding mask: the
 *   reference has none), ctx[b,:] = sum_t w[b,t] enc[b,t,:].
 *   q    [B][H]      h_top W_h^T of this step (W_a = [W_h | W_e]; tg_gemm_nt)
 *   keys [B][Te][H]  enc W_e^T + b_a, once per forward (tg_gemm_nt);  enc [B][Te][H];  v [H]
 *   w    [B][Te];    ctx [B][.] with row stride ctx_ld >= H floats (it can sit inside a concatenated input)
 * backward: dctx (row stride dctx_ld), the step's saved q and w -> dq [B][H] (written); dkeys_acc, denc_acc [B][Te][H] and dv_rows [B][H]
 * ACCUMULATE (one call per decoder step into the same buffers; the caller zeroes them and reduces dv_rows over the rows with tg_colsum).  e is
 * recomputed, not taped.  One workgroup owns one batch row: no float atomics, results are bit-identical from run to run.
 * Envelope: B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320; outside it the entries return non-zero, set tg_last_error ("envelope") and
 * launch nothing; tg_attn_step_supported writes 1 / 0 for a shape of positive sizes.  keys, enc, dkeys_acc, denc_acc: 16-byte aligned. */
int tg_attn_step_supported(int32_t B, int32_t Te, int32_t H, int32_t* supported);
int tg_attn_step_forward(const float* q, const float* keys, const float* enc, const float* v, float* w, float* ctx, int64_t ctx_ld, int32_t B,
                         int32_t Te, int32_t H, void* stream);
int tg_attn_step_backward(const float* dctx, int64_t dctx_ld, const float* q, const float* w, const float* keys, const float* enc, const float* v,
                          float* dq, float* dkeys_acc, float* denc_acc, float* dv_rows, int32_t B, int32_t Te, int32_t H, void* stream);

/* ---- Eval-mode decoder loop of the Seq2Seq baseline in ONE launch (csrc/seq2seq_decode.hip; model/seq2seq_net.py:241-252), one workgroup per
 * batch row: BatchNorm on running statistics, no dropout, so no row depends on another and no workgroup waits on another.
 *   enc, keys [B][Te][H] (keys = enc W_e^T + b_a by tg_gemm_nt, once per forward; both 16-byte aligned);  te_len: device int64 [B] or NULL --
 *   the softmax of row b runs over its first te_len[b] positions (NULL: all Te, the padded-batch semantics of training; entries are clamped
 *   to [1, Te], the caller validates them);  h0 [n_layers][B][H];  poses [B][pose_frames][Pd], pose_frames >= max(n_pre, 1);  z [B][Z] / spk
 *   [B][S8] or NULL when Z / S8 = 0;  w_attn [H][2H] (W_h = its left half), v [H];  w_pre [H][Pd + Z + H + S8], b_pre [H];  bn_*: gamma, beta,
 *   running mean and variance [H], folded once per launch;  gru_params: a table of 4 n_layers pointers, w_ih [3H][H], w_hh [3H][H], b_ih [3H],
 *   b_hh [3H] of layer 0, then of layer 1, ...;  w_out [Po][H], b_out [Po].  Weight rows need no alignment beyond 4 bytes.
 *   outputs [B][n_frames][Po]: frame 0 = poses[:, 0, :Po], frame t = the decoder's output, whose input pose is seed pose t - 1 while
 *   t - 1 < max(n_pre, 1), else its own previous output;  h_n [n_layers][B][H];  attn_w [n_frames-1][B][Te] or NULL, exact zeros at positions
 *   >= te_len[b].  fp32 FMA, libm expf / tanhf, the GRU cell of gru_step.hpp; every sum in a fixed order that does not depend on B or on the
 *   row's place in the batch.
 * Envelope: B >= 1, 1 <= Te <= 128, H % 4 == 0, 8 <= H <= 320, 1 <= n_layers <= 4, n_frames >= 2, 0 <= n_pre <= n_frames, Po == Pd or
 * n_frames == 2, 1 <= Po <= Pd, Pd + Z + H + S8 <= 1024 (the row's state lives in LDS); outside it tg_seq2seq_decode_eval returns non-zero,
 * sets tg_last_error ("envelope") and launches nothing; tg_seq2seq_decode_supported writes 1 / 0 for positive sizes. */
int tg_seq2seq_decode_supported(int32_t B, int32_t Te, int32_t H, int32_t n_layers, int32_t n_frames, int32_t n_pre, int32_t Pd, int32_t Po,
                                int32_t Z, int32_t S8, int32_t* supported);
int tg_seq2seq_decode_eval(const float* enc, const float* keys, const void* te_len, const float* h0, const float* poses, int32_t pose_frames,
                           const float* z, const float* spk, const float* w_attn, const float* v, const float* w_pre, const float* b_pre,
                           const float* bn_gamma, const float* bn_beta, const float* bn_mean, const float* bn_var, float bn_eps,
                           const void* const* gru_params, const float* w_out, const float* b_out, float* outputs, float* h_n, float* attn_w,
                           int32_t B, int32_t Te, int32_t H, int32_t n_layers, int32_t n_frames, int32_t n_pre, int32_t Pd, int32_t Po, int32_t Z,
                           int32_t S8, void* stream);

/* ---- Eval-mode recurrence of one GRU layer with per-row lengths in ONE launch (csrc/seq2seq_encode.hip; the Seq2Seq text encoder,
 * model/seq2seq_net.py:14-56): the contract of tg_gru_seq_forward without a tape, one workgroup per (batch row, direction), the state in LDS,
 * W_hh read from L2 every step; no workgroup waits on another.
 *   gi [D][B][T][3H];  w_hh_* [3H][H] (16-byte aligned), b_hh_* [3H] per direction (the reverse pair is ignored at D = 1);  h0 [D][B][H] or
 *   NULL (zeros);  lengths: device int64 [B] or NULL (every row T);  y [B][T][D H], exact zeros at t >= lengths[b], written by the kernel;
 *   h_n [D][B][H], bit for bit y[b][len - 1][:H] and y[b][0][H:];  the reverse direction starts at len - 1.  A lengths entry outside [1, T]
 *   skips the row (y = 0, h_n = h0) and sets *flag (int32, device memory, or NULL); nothing outside the row is touched.  fp32 FMA, the cell
 *   of gru_step.hpp; every sum in an order fixed by H alone: a row's result does not depend on B, on its place in the batch or on T.
 * Envelope: D in {1, 2}, B >= 1, 1 <= T <= 128, H % 4 == 0, 8 <= H <= 320; outside it tg_seq2seq_encode_eval returns non-zero, sets
 * tg_last_error ("envelope") and launches nothing; tg_seq2seq_encode_supported writes 1 / 0 for positive sizes. */
int tg_seq2seq_encode_supported(int32_t B, int32_t T, int32_t H, int32_t D, int32_t* supported);
int tg_seq2seq_encode_eval(const float* gi, const float* w_hh_fwd, const float* w_hh_rev, const float* b_hh_fwd, const float* b_hh_rev,
                           const float* h0, const void* lengths, float* y, float* h_n, int32_t* flag, int32_t B, int32_t T, int32_t H, int32_t D,
                           void* stream);

/* ---- Seq2Seq training loss and gradient clip (csrc/losses.hip; train_eval/train_seq2seq.py:6-33, 48)
 * tg_seq2seq_loss: custom_loss forward and d_output in one pass over output, target [B][T][P]:
 *   w_reg mean((o - t)^2) + w_cont sum_n |o[:, n] - o[:, n-1]| / numel - w_var sum_{b,p} ||o[b, :, p]||_2 / numel   (norm over the TIME axis)
 * fp64 sums in a fixed order; ws: 3 B doubles; scalars[0..3] = the three weighted terms and their total; subgradients: sign(0) = 0, and 0 for
 * a column whose norm is exactly 0.
 * tg_sumsq_accumulate: total[0] += sum g^2 (ws: 256 doubles of scratch; fixed order).  tg_clip_scale: out[0] = min(1, max_norm /
 * (sqrt(total) + 1e-6)) (torch.nn.utils.clip_grad_norm_), out[1] = sqrt(total).  tg_scale_by: x *= scale[0] (a device scalar: no host read
 * between the backward and the optimiser). */
int tg_seq2seq_loss(const float* output, const float* target, int32_t B, int32_t T, int32_t P, float w_reg, float w_cont, float w_var, double* ws,
                    float* scalars, float* d_output, void* stream);
int tg_sumsq_accumulate(const float* g, int64_t n, double* ws, double* total, void* stream);
int tg_clip_scale(const double* total, float max_norm, float* out, void* stream);
int tg_scale_by(float* x, int64_t n, const float* scale, void* stream);

/* ---- latent-head MLPs of the joint-embedding baseline (csrc/latent_head.hip; model/embedding_net.py:138-143, 230-259)
 * Linear(K0, N1) -> BatchNorm1d(N1) over the B rows -> act(slope: 0 ReLU, 1 identity) -> Linear(N1, N2) [-> fc_mu, fc_logvar (N2 x N2) ->
 * z = mu + eps exp(logvar / 2) when Wmu != NULL], ONE launch of one workgroup each way, no atomics, fixed summation order.
 * x is read with row stride ldx (the last step of a [B][T][K0] GRU output: x + (T - 1) K0, ldx = T K0); the result (z with the tail, the
 * second linear's output without) is written with row stride ldo (a column block of a wider row).  Train mode: batch statistics in fp64, the
 * biased variance normalises, the unbiased one feeds running_var (momentum), *nbt += 1; eval mode: the running statistics.
 * tg_latent_head_fwd leaves for the backward: h1 [B][N1] (pre-BatchNorm), stats [2 N1] DOUBLES (mean, 1 / sqrt(var + eps): the BatchNorm backward cancels almost completely at B = 2), and with the tail h2 [B][N2],
 * mu, logvar, eps [B][N2] (eps is READ when rng_state == NULL, otherwise WRITTEN: element i of tg_normal(eps, B N2, rng_state, site));
 * act_ws [B][N1] is scratch.  tg_latent_head_bwd: dout with row stride ldo, optional direct gradients dmu / dlv [B][N2] (tail), ws of
 * 2 B N1 + 3 B N2 floats; every gradient is WRITTEN (not accumulated); dx (optional) with row stride lddx.
 * Envelope: 1 <= B <= 512 (B >= 2 in train mode), 1 <= K0 <= 384, 1 <= N1 <= 256, 1 <= N2 <= 64; outside it both return non-zero, set
 * tg_last_error ("envelope") and launch nothing; tg_latent_head_supported writes 1 / 0. */
int tg_latent_head_supported(int32_t B, int32_t K0, int32_t N1, int32_t N2, int32_t training, int32_t* supported);
int tg_latent_head_fwd(const float* x, int64_t ldx, const float* W1, const float* b1, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, int64_t* nbt, const float* W2, const float* b2, const float* Wmu,
                       const float* bmu, const float* Wlv, const float* blv, float* eps, const uint64_t* rng_state, uint32_t site,
                       float* out, int64_t ldo, float* h1, float* act_ws, double* stats, float* h2, float* mu, float* logvar, int32_t B,
                       int32_t K0, int32_t N1, int32_t N2, int32_t training, float slope, float bn_eps, float momentum, void* stream);
int tg_latent_head_bwd(const float* dout, int64_t ldo, const float* dmu, const float* dlv, const float* x, int64_t ldx, const float* W1,
                       const float* gamma, const float* beta, const float* W2, const float* Wmu, const float* Wlv, const float* eps,
                       const float* h1, const double* stats, const float* h2, const float* logvar, float* ws, float* dW1, float* db1,
                       float* dgamma, float* dbeta, float* dW2, float* db2, float* dWmu, float* dbmu, float* dWlv, float* dblv, float* dx,
                       int64_t lddx, int32_t B, int32_t K0, int32_t N1, int32_t N2, int32_t training, float slope, void* stream);

/* ---- variational tail of the pose encoder (csrc/vae_latent.hip; model/embedding_net.py:67-82 with variational_encoding=True, the KL term
 * of train_feature_extractor.py:74-79 and train_eval/train_joint_embed.py:30-36).  ONE launch of one workgroup each, no atomics, every sum
 * one fp64 chain in a fixed order (two runs are bit identical).
 * tg_vae_latent_fwd: f3 [B][32] (pose_encoder.out_net.6's output), Wmu / Wlv [32][32], bmu / blv [32] -> mu, logvar, z = mu + eps
 * exp(logvar / 2) [B][32] and *kld = -0.5 sum(1 + logvar - mu^2 - exp(logvar)) over the batch, in fp64 from the fp32 mu / logvar written.
 * eps [B][32] is READ when rng_state == NULL, otherwise WRITTEN: element i of tg_normal(eps, 32 B, rng_state, site).  Row b of the results
 * depends on row b of the inputs only; its bits do not change with B.
 * tg_vae_latent_bwd: dmu_total = dz + w mu + dmu, dlv_total = dz eps 0.5 exp(logvar / 2) + w 0.5 (exp(logvar) - 1) + dlv (w: the weight of the
 * KL term, may be 0; dz NULL: no gradient through z; dmu / dlv: optional direct gradients of mu / logvar) -> dWmu, dbmu, dWlv, dblv and
 * df3 = dmu_total Wmu + dlv_total Wlv, all WRITTEN (not accumulated).  ws: 64 B floats.  f3, ws 16-byte aligned.
 * tg_vae_kld: the KL term of any latent mu, logvar [B][N] (the context encoder's): *kld as above and, when dmu / dlv != NULL, its gradient
 * dmu = w mu, dlv = w 0.5 (exp(logvar) - 1).
 * Envelope: 1 <= B <= 1024 (tg_vae_kld: B N <= 65536); outside it the entries return non-zero, set tg_last_error ("envelope") and launch
 * nothing. */
int tg_vae_latent_fwd(const float* f3, const float* Wmu, const float* bmu, const float* Wlv, const float* blv, float* eps,
                      const uint64_t* rng_state, uint32_t site, float* mu, float* logvar, float* z, double* kld, int32_t B, void* stream);
int tg_vae_latent_bwd(const float* dz, const float* dmu, const float* dlv, const float* mu, const float* logvar, const float* eps,
                      const float* f3, const float* Wmu, const float* Wlv, float w, float* ws, float* dWmu, float* dbmu, float* dWlv,
                      float* dblv, float* df3, int32_t B, void* stream);
int tg_vae_kld(const float* mu, const float* logvar, int32_t B, int32_t N, float w, double* kld, float* dmu, float* dlv, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIMODAL_HIP_H */
