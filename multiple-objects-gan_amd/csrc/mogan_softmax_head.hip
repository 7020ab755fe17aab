// mogan_softmax_head.hip -- the sums the Inception Score of DESIGN.md section 9o is computed from (attngan/inception_score.py has the
// whole definition): for n pool codes x (n, D), a classifier head w (C, D), bias (C) -- all fp32, widened exactly -- and S contiguous
// splits of the rows, split s = [floor(s n / S), floor((s + 1) n / S)),
//
//   z[i][y]    = <x_i, w_y> + bias[y]                      everything after the loads in fp64
//   row_lse[i] = log sum_y exp(z[i][y])                    the maximum subtracted
//   row_h[i]   = sum_y p[i][y] (z[i][y] - row_lse[i])      p[i][y] = exp(z[i][y] - row_lse[i]); a p of exactly 0 adds exactly 0
//   psum[s][y] = sum_{i in split s} p[i][y]
//
// The reference repository has no code for this.  No z, no p ever reaches memory.
//
// softmax_head_kernel: one 4-wave block per STRIPE of 64 rows; the stripes of a split start at the split's first row, grid
// (stripe of the split, split), blocks past a split's last stripe leave at once.  The block walks the ceil(C / 64) column tiles of
// the head TWICE; the tile of <x_i, w_y> is gram64_tile of csrc/mogan_gram64.h on two row panels (64 code rows, 64 head rows), the
// reduction along the features in index order in every accumulator, rows past the stripe, head rows past C and features past D
// entering as zeros -- so a logit's bits depend on its code row and its head row only, and are the same in both walks.
//   Walk 1: a lane keeps, per row it holds (8) and over its own columns (2 per tile), a running maximum m and Z = sum exp(z - m),
//     rescaled by exp(m - z) when a new maximum arrives.  The row's 32 pairs (column slot = (wave & 1) * 16 + (lane & 15)) meet in
//     LDS; one thread per row takes M = max m and adds Z exp(m - M) in slot order (a slot without a column adds nothing):
//     row_lse = M + log(sum).
//   Walk 2: lp = z - row_lse, p = exp(lp); a lane adds p lp per row in (tile, column) order, the 32 slots are added per row in slot
//     order -> row_h.  Per column the lane adds its 8 rows' p (rows past the stripe as 0) in register order, the 16-lane groups meet
//     in a butterfly (xor 16, 32), the two waves of a column in LDS: ONE double per (stripe, class) to ws[split][stripe][class].
// Which wave, lane and register holds a row decides nothing about the order in which its columns are added, so row_lse and row_h
// depend on the row, the head, D and C only; a column's sum depends on the stripe's rows in order, and a stripe is rows
// [64 t, 64 t + 64) OF ITS SPLIT.
//
// softmax_head_finish_kernel: one thread per (split, class) adds the split's stripe partials in stripe order.  psum[s] is therefore,
// bit for bit, what the S = 1 call on the split's rows alone gives.  No atomics: the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mogan_gram64.h"

namespace {

constexpr int S_MAX = 65535;                 // grid.y
constexpr int C_MAX = 1 << 20;               // classes: ceil(C / 256) blocks of the finish grid, and 8 S maxT C stays below 2^63
constexpr int SLOTS = 32;                    // lanes that share a row: 2 waves x 16 lanes

__host__ __device__ inline long long split_start(long long n, int S, int s) { return (long long)s * n / S; }   // s n < 2^47

static inline long long stripes_per_split(long long n, int S) {
    const long long most = (n + S - 1) / S;                 // rows of the fullest split
    return (most + CT - 1) / CT;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void softmax_head_kernel(const float* __restrict__ x, long long n, int D,
                                                          const float* __restrict__ w, const float* __restrict__ bias, int C, int S,
                                                          int maxT, double* __restrict__ row_lse, double* __restrict__ row_h,
                                                          double* __restrict__ ws) {
    __shared__ GramLds sm;
    __shared__ double lse_s[CT];
    __shared__ double colred[2][CT];
    const int split = blockIdx.y, t = blockIdx.x;
    const long long lo = split_start(n, S, split), hi = split_start(n, S, split + 1);
    const long long r0 = lo + (long long)t * CT;
    if (r0 >= hi) return;                                    // the whole block: this split has fewer stripes
    const int rows = hi - r0 < CT ? (int)(hi - r0) : CT;
    const int Tc = (C + CT - 1) / CT;
    const int tid = threadIdx.x;
    const double NEG_INF = -__builtin_huge_val();

    const int sr = RowPanels<VEC>::stage_row();
    const bool va = sr < rows;
    const float* xa = x + (size_t)(va ? r0 + sr : r0) * D;
    const GramLane ln;
    const int slot = ln.wc * 16 + ln.lc;
    // the staging image is free between two tiles: [row][slot][2] for the rows' partial results (4096 of its 5120 doubles)
    double (*part)[SLOTS][2] = reinterpret_cast<double (*)[SLOTS][2]>(&sm[0][0][0]);
    f64x4 acc[2][2];

    // ---- walk 1: the rows' log-sum-exp
    double mx[2][4], zs[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) { mx[m][j] = NEG_INF; zs[m][j] = 0.0; }
    for (int ct = 0; ct < Tc; ++ct) {
        const int c0 = ct * CT, wrow = c0 + sr;
        const bool vb = wrow < C;
        RowPanels<VEC> src(xa, va, w + (size_t)(vb ? wrow : 0) * D, vb, D, false);
        gram64_tile(src, sm, acc);
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int col = ln.col(c0, nn);
            if (col >= C) continue;
            const double b = (double)bias[col];
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double z = acc[m][nn][j] + b;
                    if (z > mx[m][j]) {
                        zs[m][j] = zs[m][j] * exp(mx[m][j] - z);
                        mx[m][j] = z;
                    }
                    zs[m][j] += exp(z - mx[m][j]);
                }
        }
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ln.row(0, m, j);
            part[r][slot][0] = mx[m][j];
            part[r][slot][1] = zs[m][j];
        }
    __syncthreads();
    if (tid < CT) {
        double M = NEG_INF;
        for (int c = 0; c < SLOTS; ++c) M = fmax(M, part[tid][c][0]);
        double Z = 0.0;
        for (int c = 0; c < SLOTS; ++c) {
            const double mc = part[tid][c][0];
            if (mc > NEG_INF) Z += part[tid][c][1] * exp(mc - M);
        }
        const double lse = M + log(Z);
        lse_s[tid] = lse;
        if (tid < rows && row_lse) row_lse[r0 + tid] = lse;
    }
    __syncthreads();

    // ---- walk 2: p = exp(z - lse); the rows' sum of p log p and the stripe's column sums of p
    double hs[2][4], lse_r[2][4];
    bool vr[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = ln.row(0, m, j);
            hs[m][j] = 0.0;
            lse_r[m][j] = lse_s[r];
            vr[m][j] = r < rows;
        }
    double* wsrow = ws + ((size_t)split * maxT + t) * C;
    for (int ct = 0; ct < Tc; ++ct) {
        const int c0 = ct * CT, wrow = c0 + sr;
        const bool vb = wrow < C;
        RowPanels<VEC> src(xa, va, w + (size_t)(vb ? wrow : 0) * D, vb, D, false);
        gram64_tile(src, sm, acc);
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int col = ln.col(c0, nn);
            const bool vc = col < C;
            const double b = vc ? (double)bias[col] : 0.0;
            double cs = 0.0;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double lp = (acc[m][nn][j] + b) - lse_r[m][j];
                    const double p = exp(lp);
                    if (vc) hs[m][j] += p == 0.0 ? 0.0 : p * lp;
                    cs += vr[m][j] ? p : 0.0;
                }
            cs += __shfl_xor(cs, 16, 64);
            cs += __shfl_xor(cs, 32, 64);
            if (ln.lk == 0) colred[ln.wr][ln.wc * 32 + nn * 16 + ln.lc] = cs;
        }
        __syncthreads();
        if (tid < CT && c0 + tid < C) wsrow[c0 + tid] = colred[0][tid] + colred[1][tid];
        // (colred is written again only behind the barriers of the next tile)
    }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) part[ln.row(0, m, j)][slot][0] = hs[m][j];
    __syncthreads();
    if (tid < rows) {
        double h = 0.0;
        for (int c = 0; c < SLOTS; ++c) h += part[tid][c][0];
        row_h[r0 + tid] = h;
    }
}

__global__ __launch_bounds__(NT) void softmax_head_finish_kernel(const double* __restrict__ ws, long long n, int C, int S, int maxT,
                                                                 double* __restrict__ psum) {
    const int split = blockIdx.y;
    const long long c = (long long)blockIdx.x * NT + threadIdx.x;
    if (c >= C) return;
    const long long rows = split_start(n, S, split + 1) - split_start(n, S, split);
    const int T = (int)((rows + CT - 1) / CT);
    const double* p = ws + (size_t)split * maxT * C + c;
    double t = 0.0;
    for (int i = 0; i < T; ++i) t += p[(size_t)i * C];
    psum[(size_t)split * C + c] = t;
}

static inline bool bad_shape(long long n, int C, int S) {
    return n < 1 || n > N_MAX || C < 1 || C > C_MAX || S < 1 || S > S_MAX || (long long)S > n;
}

}  // namespace

extern "C" {

size_t mogan_softmax_head_ws_bytes(long long n, int C, int S) {
    if (bad_shape(n, C, S)) return 0;
    return (size_t)S * (size_t)stripes_per_split(n, S) * (size_t)C * sizeof(double);
}

int mogan_softmax_head_f64(const float* x, long long n, int D, const float* w, const float* bias, int C, int S, double* row_lse,
                           double* row_h, double* psum, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!x || !w || !bias || !row_h || !psum || bad_shape(n, C, S) || D < 1 || D > D_MAX) return MOGAN_ERR_SHAPE;
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias) & 3) != 0 ||
        (((uintptr_t)row_lse | (uintptr_t)row_h | (uintptr_t)psum) & 7) != 0)
        return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_softmax_head_ws_bytes(n, C, S)) return MOGAN_ERR_WS;
    const long long maxT = stripes_per_split(n, S);          // <= 2^25
    const bool vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0;
    const dim3 grid((unsigned)maxT, S);
    if (vec)
        hipLaunchKernelGGL(softmax_head_kernel<true>, grid, dim3(NT), 0, stream, x, n, D, w, bias, C, S, (int)maxT, row_lse, row_h,
                           (double*)ws);
    else
        hipLaunchKernelGGL(softmax_head_kernel<false>, grid, dim3(NT), 0, stream, x, n, D, w, bias, C, S, (int)maxT, row_lse, row_h,
                           (double*)ws);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(softmax_head_finish_kernel, dim3((C + NT - 1) / NT, S), dim3(NT), 0, stream, (const double*)ws, n, C, S,
                       (int)maxT, psum);
    return ok_launch();
}

}  // extern "C"
