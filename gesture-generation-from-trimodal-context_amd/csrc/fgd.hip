// Frechet gesture distance on the device (model/embedding_space_evaluator.py:74-156): streaming fp64 moments of the autoencoder's latent features
// and the 32 x 32 symmetric finish, so that a validation pass makes no host read until the score is asked for and stores nothing per sample.
//
// State (doubles; tg_fgd_state_doubles(D)): [0] first-push flag, [1] pushes, [2] sum of (recon_err_fake - recon_err_real), [3] sum over rows of
//   sum_j |real - generated|, [4, 4 + D) the pivot K; then per set (0 real, 1 generated) n, sum (x - K) [D], sum (x - K)(x - K)^T [D][D]; then the
//   push workspace: the pivot of a first push [D] and FG_MAX_WG partial blocks {sum0 [D], outer0 [D][D], sum1 [D], outer1 [D][D], l1}.
// fgd_partial_kernel -- workgroup w owns rows [256 c, 256 c + 256) for c = w, w + grid, ...; 64 rows at a time go through LDS as doubles minus the
//   pivot; thread t owns entries (t / 8, 4 (t % 8) .. + 3) of both outer products in registers, threads 0 .. 63 the column sums, the row L1
//   distances are added in row order.  On a first push (flag 0) every workgroup forms the pivot = mean of the real batch itself, in one fixed
//   order, so all of them subtract the same doubles; workgroup 0 leaves it in the workspace.
// fgd_reduce_kernel  -- adds the partial blocks to the state entry by entry in workgroup order; its workgroup 0 adopts the pivot, raises the flag
//   and counts.  No floating-point atomics anywhere: two runs over the same pushes leave bit-identical states.
// fgd_scores_kernel  -- one workgroup: mu / cov (ddof 1) from the shifted sums (or given moments), cyclic Jacobi with round-robin parallel
//   ordering (the D / 2 disjoint rotations of a step computed together, applied to columns, then to rows) on S1 with eigenvectors,
//   R = V sqrt(max(w, 0)) V^T, M = R S2 R symmetrised, Jacobi again for its eigenvalues; three 8 KB fp64 matrices in LDS.
#include "common.hpp"

#include <math.h>

namespace tg {

constexpr int FG_MAXD = 32, FG_THREADS = 256, FG_ROWS_PER_WG = 256, FG_MAX_WG = 16, FG_SUB = 64, FG_HDR = 4, FG_SWEEP_CAP = 30;
constexpr int FG_LD = FG_MAXD;

__host__ __device__ inline long fg_set_doubles(int D) { return 1 + D + (long)D * D; }
__host__ __device__ inline long fg_set_off(int D, int s) { return FG_HDR + D + s * fg_set_doubles(D); }
__host__ __device__ inline long fg_head_doubles(int D) { return FG_HDR + D + 2 * fg_set_doubles(D); }
__host__ __device__ inline long fg_part_doubles(int D) { return 2 * (D + (long)D * D) + 1; }
__host__ __device__ inline long fg_state_doubles(int D) { return fg_head_doubles(D) + D + FG_MAX_WG * fg_part_doubles(D); }

__global__ __launch_bounds__(FG_THREADS) void fgd_partial_kernel(double* __restrict__ state, const float* __restrict__ real,
                                                                 const float* __restrict__ gen, int B, int D) {
    __shared__ double xs[3][FG_SUB][FG_MAXD + 1];             // real - K, generated - K, |real - generated|
    __shared__ double Ks[FG_MAXD];
    __shared__ double red[8][FG_MAXD];
    __shared__ double l1row[FG_SUB];
    const int t = threadIdx.x;
    double* __restrict__ ws = state + fg_head_doubles(D);
    for (int e = t; e < 3 * FG_SUB * (FG_MAXD + 1); e += FG_THREADS) (&xs[0][0][0])[e] = 0.0;
    // first push: pivot = mean of this real batch.  Every workgroup (up to 16) reads the WHOLE batch for it, eight threads per column, in the same
    // order -- redundant on purpose: all workgroups then subtract bit-identical doubles without a grid-wide step or a third launch.  The cost
    // grows with B (B x D floats per workgroup, from L2 after the first) and is paid once per evaluator; negligible at B = 128, ~0.5 MB per
    // workgroup for a one-shot 4 K-row fgd_scores_device call.  A pre-pass kernel would be the thing to add if one-shot calls grew much larger.
    if (state[0] == 0.0) {
        const int j = t & 31, g = t >> 5;
        double a = 0.0;
        if (j < D)
            for (long r = g; r < B; r += 8) a += (double)real[r * D + j];
        red[g][j] = a;
        __syncthreads();
        if (t < D) {
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) s += red[q][t];
            Ks[t] = s / (double)B;
            if (blockIdx.x == 0) ws[t] = Ks[t];
        }
    } else if (t < D) {
        Ks[t] = state[FG_HDR + t];
    }
    const int i = t >> 3, j0 = (t & 7) * 4;
    const int cset = (t >> 5) & 1, ccol = t & 31;
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    double cs = 0.0, l1 = 0.0;
    for (long c0 = (long)blockIdx.x * FG_ROWS_PER_WG; c0 < B; c0 += (long)gridDim.x * FG_ROWS_PER_WG) {
        const int crow = B - c0 < FG_ROWS_PER_WG ? (int)(B - c0) : FG_ROWS_PER_WG;
        for (int s0 = 0; s0 < crow; s0 += FG_SUB) {
            const int nr = crow - s0 < FG_SUB ? crow - s0 : FG_SUB;
            __syncthreads();                                  // (the pivot is in LDS; the previous rows' reads are done)
            for (int e = t; e < nr * D; e += FG_THREADS) {
                const int r = e / D, j = e - r * D;
                const long gi = (c0 + s0 + r) * D + j;
                const double a = (double)real[gi], b = (double)gen[gi];
                xs[0][r][j] = a - Ks[j];
                xs[1][r][j] = b - Ks[j];
                xs[2][r][j] = fabs(a - b);
            }
            __syncthreads();
            if (i < D)
                for (int r = 0; r < nr; ++r) {
                    const double x0 = xs[0][r][i], x1 = xs[1][r][i];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        acc[0][q] += x0 * xs[0][r][j0 + q];
                        acc[1][q] += x1 * xs[1][r][j0 + q];
                    }
                }
            if (t < 64 && ccol < D)
                for (int r = 0; r < nr; ++r) cs += xs[cset][r][ccol];
            if (t >= 64 && t < 64 + nr) {
                double a = 0.0;
                for (int j = 0; j < D; ++j) a += xs[2][t - 64][j];
                l1row[t - 64] = a;
            }
            __syncthreads();
            if (t == 128)
                for (int r = 0; r < nr; ++r) l1 += l1row[r];
        }
    }
    const long half = D + (long)D * D;
    double* __restrict__ part = ws + D + (long)blockIdx.x * fg_part_doubles(D);
    if (i < D) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (j0 + q < D) {
                part[D + (long)i * D + j0 + q] = acc[0][q];
                part[half + D + (long)i * D + j0 + q] = acc[1][q];
            }
    }
    if (t < 64 && ccol < D) part[cset * half + ccol] = cs;
    if (t == 128) part[2 * half] = l1;
}

__global__ __launch_bounds__(FG_THREADS) void fgd_reduce_kernel(double* __restrict__ state, int n_wg, int B, int D, const float* __restrict__ err_real,
                                                                const float* __restrict__ err_fake) {
    const int t = threadIdx.x;
    const long half = D + (long)D * D, P = fg_part_doubles(D);
    const double* __restrict__ ws = state + fg_head_doubles(D);
    const long e = (long)blockIdx.x * FG_THREADS + t;
    if (e < P) {
        double a = 0.0;
        for (int w = 0; w < n_wg; ++w) a += ws[D + (long)w * P + e];
        const long at = e < half ? fg_set_off(D, 0) + 1 + e : (e < 2 * half ? fg_set_off(D, 1) + 1 + (e - half) : 3);
        state[at] += a;
    }
    if (blockIdx.x == 0) {
        const bool first = state[0] == 0.0;
        __syncthreads();
        if (first && t < D) state[FG_HDR + t] = ws[t];
        if (t == 0) {
            state[0] = 1.0;
            state[1] += 1.0;
            double d = 0.0;
            if (err_fake) d += (double)err_fake[0];
            if (err_real) d -= (double)err_real[0];
            state[2] += d;
            state[fg_set_off(D, 0)] += (double)B;
            state[fg_set_off(D, 1)] += (double)B;
        }
    }
}

// sum of squares of the leading m x m block (all of it, or off the diagonal), every thread gets the result; fixed order
__device__ double fg_sumsq(const double* __restrict__ A, int m, bool off_only, double* __restrict__ red) {
    const int t = threadIdx.x;
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t * 4 + q, r = e >> 5, c = e & 31;
        if (r < m && c < m && !(off_only && r == c)) a += A[e] * A[e];
    }
    red[t] = a;
    __syncthreads();
    for (int s = FG_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double v = red[0];
    __syncthreads();
    return v;
}

// cyclic Jacobi on the symmetric leading m x m block of A (m even), eigenvalues left on the diagonal, eigenvectors in the columns of V (or V null);
// returns the sweeps used, -1 - sweeps where the cap was reached
__device__ int fg_jacobi(double* __restrict__ A, double* __restrict__ V, int m, double* __restrict__ red, double* __restrict__ rc, double* __restrict__ rs,
                         double* __restrict__ rpp, double* __restrict__ rqq, int* __restrict__ rp, int* __restrict__ rq) {
    const int t = threadIdx.x, h = m >> 1;
    const double thresh = 2.220446049250313e-16 * sqrt(fg_sumsq(A, m, false, red));
    int sweeps = 0;
    for (;;) {
        const double off = sqrt(fg_sumsq(A, m, true, red));
        if (off <= thresh) return sweeps;
        if (sweeps == FG_SWEEP_CAP) return -1 - sweeps;
        for (int step = 0; step < m - 1; ++step) {
            if (t < h) {                                      // round-robin: player m - 1 stays, the others move round
                int p = t == 0 ? m - 1 : (step + t) % (m - 1), q = t == 0 ? step : (step - t + m - 1) % (m - 1);
                if (p > q) { const int x = p; p = q; q = x; }
                const double app = A[p * FG_LD + p], aqq = A[q * FG_LD + q], apq = A[p * FG_LD + q];
                double c = 1.0, s = 0.0, npp = app, nqq = aqq;
                if (apq != 0.0) {
                    const double th = (aqq - app) / (2.0 * apq);
                    const double tn = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    c = 1.0 / sqrt(tn * tn + 1.0);
                    s = tn * c;
                    npp = app - tn * apq;                     // the rotated diagonal in the form that keeps the trace (Rutishauser)
                    nqq = aqq + tn * apq;
                }
                rc[t] = c; rs[t] = s; rpp[t] = npp; rqq[t] = nqq; rp[t] = p; rq[t] = q;
            }
            __syncthreads();
            for (int e = t; e < h * m; e += FG_THREADS) {     // columns p, q of A (and V)
                const int k = e / m, r = e - k * m, p = rp[k], q = rq[k];
                const double c = rc[k], s = rs[k];
                const double a = A[r * FG_LD + p], b = A[r * FG_LD + q];
                A[r * FG_LD + p] = c * a - s * b;
                A[r * FG_LD + q] = s * a + c * b;
                if (V) {
                    const double va = V[r * FG_LD + p], vb = V[r * FG_LD + q];
                    V[r * FG_LD + p] = c * va - s * vb;
                    V[r * FG_LD + q] = s * va + c * vb;
                }
            }
            __syncthreads();
            for (int e = t; e < h * m; e += FG_THREADS) {     // rows p, q; the rotated pair itself is set to zero, its diagonal taken from above
                const int k = e / m, col = e - k * m, p = rp[k], q = rq[k];
                const double c = rc[k], s = rs[k];
                const double a = A[p * FG_LD + col], b = A[q * FG_LD + col];
                const bool live = s != 0.0;
                A[p * FG_LD + col] = (live && col == q) ? 0.0 : ((live && col == p) ? rpp[k] : c * a - s * b);
                A[q * FG_LD + col] = (live && col == p) ? 0.0 : ((live && col == q) ? rqq[k] : s * a + c * b);
            }
            __syncthreads();
        }
        ++sweeps;
    }
}

// x_ij = x_ji = their mean over the whole 32 x 32 tile
__device__ void fg_symmetrise(double* __restrict__ A) {
    for (int e = threadIdx.x; e < FG_MAXD * FG_MAXD; e += FG_THREADS) {
        const int r = e >> 5, c = e & 31;
        if (r < c) {
            const double v = 0.5 * (A[r * FG_LD + c] + A[c * FG_LD + r]);
            A[r * FG_LD + c] = v;
            A[c * FG_LD + r] = v;
        }
    }
    __syncthreads();
}

// the covariance of one set into the (zero-padded) tile: from the shifted sums of the state, or the given matrix
__device__ void fg_load_cov(double* __restrict__ A, const double* __restrict__ set, const double* __restrict__ given, int D) {
    const double n = set ? set[0] : 0.0;
    for (int e = threadIdx.x; e < FG_MAXD * FG_MAXD; e += FG_THREADS) {
        const int r = e >> 5, c = e & 31;
        double v = 0.0;
        if (r < D && c < D) v = set ? (set[1 + D + (long)r * D + c] - set[1 + r] * set[1 + c] / n) / (n - 1.0) : given[(long)r * D + c];
        A[e] = v;
    }
    __syncthreads();
    fg_symmetrise(A);
}

// state != null: S1 = the generated set, S2 = the real set (fgd.fgd_scores's order); else the given moments
__global__ __launch_bounds__(FG_THREADS) void fgd_scores_kernel(const double* __restrict__ state, const double* __restrict__ mu1, const double* __restrict__ S1,
                                                                const double* __restrict__ mu2, const double* __restrict__ S2, int D, double* __restrict__ out) {
    __shared__ double A[FG_MAXD * FG_LD], V[FG_MAXD * FG_LD], T[FG_MAXD * FG_LD];
    __shared__ double red[FG_THREADS], rc[FG_MAXD / 2], rs[FG_MAXD / 2], rpp[FG_MAXD / 2], rqq[FG_MAXD / 2], sq[FG_MAXD];
    __shared__ int rp[FG_MAXD / 2], rq[FG_MAXD / 2];
    const int t = threadIdx.x, m = (D + 1) & ~1;
    const double* set_r = state ? state + fg_set_off(D, 0) : nullptr;
    const double* set_g = state ? state + fg_set_off(D, 1) : nullptr;
    const double n = state ? set_r[0] : 0.0;
    double status = 0.0;
    if (state && n < 2.0) {                                   // no covariance yet: only the paired distance means anything
        if (t == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            out[0] = nan;
            out[1] = n > 0.0 ? state[3] / n : nan;
            out[2] = n;
            out[3] = state[1] > 0.0 ? state[2] / state[1] : nan;
            for (int q = 4; q < 10; ++q) out[q] = nan;
            out[10] = 2.0;
        }
        return;
    }
    fg_load_cov(A, set_g, S1, D);
    for (int e = t; e < FG_MAXD * FG_LD; e += FG_THREADS) V[e] = (e >> 5) == (e & 31) ? 1.0 : 0.0;
    double tr1 = 0.0, tr2 = 0.0, d2 = 0.0;
    if (t == 0) {
        for (int j = 0; j < D; ++j) {
            tr1 += A[j * FG_LD + j];
            const double d = state ? set_g[1 + j] / set_g[0] - set_r[1 + j] / set_r[0] : mu1[j] - mu2[j];
            d2 += d * d;
        }
    }
    __syncthreads();
    const int sw1 = fg_jacobi(A, V, m, red, rc, rs, rpp, rqq, rp, rq);
    if (t < FG_MAXD) sq[t] = sqrt(fmax(A[t * FG_LD + t], 0.0));
    __syncthreads();
    for (int e = t; e < FG_MAXD * FG_LD; e += FG_THREADS) {   // R = V sqrt(w) V^T
        const int r = e >> 5, c = e & 31;
        double a = 0.0;
        for (int k = 0; k < FG_MAXD; ++k) a += V[r * FG_LD + k] * sq[k] * V[c * FG_LD + k];
        T[e] = a;
    }
    __syncthreads();
    fg_load_cov(A, set_r, S2, D);
    if (t == 0)
        for (int j = 0; j < D; ++j) tr2 += A[j * FG_LD + j];
    for (int e = t; e < FG_MAXD * FG_LD; e += FG_THREADS) {   // V = R S2
        const int r = e >> 5, c = e & 31;
        double a = 0.0;
        for (int k = 0; k < FG_MAXD; ++k) a += T[r * FG_LD + k] * A[k * FG_LD + c];
        V[e] = a;
    }
    __syncthreads();
    for (int e = t; e < FG_MAXD * FG_LD; e += FG_THREADS) {   // A = (R S2) R
        const int r = e >> 5, c = e & 31;
        double a = 0.0;
        for (int k = 0; k < FG_MAXD; ++k) a += V[r * FG_LD + k] * T[k * FG_LD + c];
        A[e] = a;
    }
    __syncthreads();
    fg_symmetrise(A);
    const int sw2 = fg_jacobi(A, nullptr, m, red, rc, rs, rpp, rqq, rp, rq);
    if (sw1 < 0 || sw2 < 0) status += 1.0;
    if (t == 0) {
        double ssum = 0.0;
        for (int j = 0; j < D; ++j) ssum += sqrt(fmax(A[j * FG_LD + j], 0.0));
        out[0] = d2 + tr1 + tr2 - 2.0 * ssum;
        out[1] = state ? state[3] / n : 0.0;
        out[2] = n;
        out[3] = state && state[1] > 0.0 ? state[2] / state[1] : 0.0;
        out[4] = tr1;
        out[5] = tr2;
        out[6] = d2;
        out[7] = ssum;
        out[8] = (double)(sw1 < 0 ? -1 - sw1 : sw1);
        out[9] = (double)(sw2 < 0 ? -1 - sw2 : sw2);
        out[10] = status;
    }
}

static bool fg_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace tg

using namespace tg;

#define FG_ALIGNED8(p) ((reinterpret_cast<uintptr_t>(p) & 7u) == 0)
#define FG_ALIGNED4(p) ((reinterpret_cast<uintptr_t>(p) & 3u) == 0)

extern "C" int tg_fgd_state_doubles(int32_t D, int64_t* doubles) {
    TG_REQUIRE(doubles, "tg_fgd_state_doubles: doubles is NULL");
    TG_REQUIRE(D >= 1 && D <= FG_MAXD, "tg_fgd_state_doubles: D = %d outside 1 .. %d", (int)D, FG_MAXD);
    *doubles = fg_state_doubles(D);
    return 0;
}

extern "C" int tg_fgd_reset(void* state, int32_t D, void* stream) {
    TG_REQUIRE(state, "tg_fgd_reset: state is NULL");
    TG_REQUIRE(D >= 1 && D <= FG_MAXD, "tg_fgd_reset: D = %d outside 1 .. %d", (int)D, FG_MAXD);
    TG_REQUIRE(FG_ALIGNED8(state), "tg_fgd_reset: state must be 8-byte aligned");
    return zero_async(state, (size_t)fg_head_doubles(D) * sizeof(double), (hipStream_t)stream);
}

extern "C" int tg_fgd_push(void* state, const float* real_feat, const float* gen_feat, int32_t B, int32_t D, const float* recon_err_real,
                           const float* recon_err_fake, void* stream) {
    TG_REQUIRE(state && real_feat && gen_feat, "tg_fgd_push: NULL pointer argument (state, real_feat, gen_feat)");
    TG_REQUIRE(D >= 1 && D <= FG_MAXD, "tg_fgd_push: D = %d outside 1 .. %d", (int)D, FG_MAXD);
    TG_REQUIRE(B >= 1, "tg_fgd_push: B = %d must be positive", (int)B);
    TG_REQUIRE(FG_ALIGNED8(state) && FG_ALIGNED4(real_feat) && FG_ALIGNED4(gen_feat) && FG_ALIGNED4(recon_err_real) && FG_ALIGNED4(recon_err_fake),
               "tg_fgd_push: misaligned pointer (state 8 bytes, features and scalars 4)");
    const int64_t sb = fg_state_doubles(D) * 8, fb = (int64_t)B * D * 4;
    TG_REQUIRE(!fg_overlap(state, sb, real_feat, fb) && !fg_overlap(state, sb, gen_feat, fb) && !(recon_err_real && fg_overlap(state, sb, recon_err_real, 4)) &&
               !(recon_err_fake && fg_overlap(state, sb, recon_err_fake, 4)), "tg_fgd_push: an input overlaps the state buffer");
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = ((int64_t)B + FG_ROWS_PER_WG - 1) / FG_ROWS_PER_WG;
    const int n_wg = (int)(chunks > FG_MAX_WG ? FG_MAX_WG : chunks);
    hipLaunchKernelGGL(fgd_partial_kernel, dim3(n_wg), dim3(FG_THREADS), 0, s, static_cast<double*>(state), real_feat, gen_feat, (int)B, (int)D);
    if (check_launch("tg_fgd_push(partials)")) return 1;
    const int r_wg = (int)((fg_part_doubles(D) + FG_THREADS - 1) / FG_THREADS);
    hipLaunchKernelGGL(fgd_reduce_kernel, dim3(r_wg), dim3(FG_THREADS), 0, s, static_cast<double*>(state), n_wg, (int)B, (int)D, recon_err_real, recon_err_fake);
    return check_launch("tg_fgd_push(reduce)");
}

extern "C" int tg_fgd_scores(const void* state, int32_t D, double* out, void* stream) {
    TG_REQUIRE(state && out, "tg_fgd_scores: NULL pointer argument (state, out)");
    TG_REQUIRE(D >= 1 && D <= FG_MAXD, "tg_fgd_scores: D = %d outside 1 .. %d", (int)D, FG_MAXD);
    TG_REQUIRE(FG_ALIGNED8(state) && FG_ALIGNED8(out), "tg_fgd_scores: misaligned pointer (8 bytes)");
    TG_REQUIRE(!fg_overlap(state, fg_state_doubles(D) * 8, out, TG_FGD_OUT_DOUBLES * 8), "tg_fgd_scores: out overlaps the state buffer");
    const double* none = nullptr;
    hipLaunchKernelGGL(fgd_scores_kernel, dim3(1), dim3(FG_THREADS), 0, (hipStream_t)stream, static_cast<const double*>(state), none, none, none, none, (int)D, out);
    return check_launch("tg_fgd_scores");
}

extern "C" int tg_fgd_from_stats(const double* mu1, const double* S1, const double* mu2, const double* S2, int32_t D, double* out, void* stream) {
    TG_REQUIRE(mu1 && S1 && mu2 && S2 && out, "tg_fgd_from_stats: NULL pointer argument");
    TG_REQUIRE(D >= 1 && D <= FG_MAXD, "tg_fgd_from_stats: D = %d outside 1 .. %d", (int)D, FG_MAXD);
    TG_REQUIRE(FG_ALIGNED8(mu1) && FG_ALIGNED8(S1) && FG_ALIGNED8(mu2) && FG_ALIGNED8(S2) && FG_ALIGNED8(out), "tg_fgd_from_stats: misaligned pointer (8 bytes)");
    const int64_t ob = TG_FGD_OUT_DOUBLES * 8, vb = (int64_t)D * 8, mb = (int64_t)D * D * 8;
    TG_REQUIRE(!fg_overlap(out, ob, mu1, vb) && !fg_overlap(out, ob, mu2, vb) && !fg_overlap(out, ob, S1, mb) && !fg_overlap(out, ob, S2, mb),
               "tg_fgd_from_stats: out overlaps an input");
    const double* none = nullptr;
    hipLaunchKernelGGL(fgd_scores_kernel, dim3(1), dim3(FG_THREADS), 0, (hipStream_t)stream, none, mu1, S1, mu2, S2, (int)D, out);
    return check_launch("tg_fgd_from_stats");
}
