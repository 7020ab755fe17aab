// mogan_stats.hip -- the fp64 moments of a set of feature codes: what the Frechet distance of DESIGN.md section 9d is computed from.
//
//   mean[j]   = (sum_n (double)x[n][j]) / N
//   cov[i][j] = (sum_n (x[n][i] - mean[i]) (x[n][j] - mean[j])) / (N - 1)              (numpy.cov(x, rowvar=False))
//
// x is fp32 (N, D), widened exactly; everything after the load is fp64.  The reference repository has no code for this.
//
// col_mean_f64_kernel: a block owns 16 columns; its 16 row groups each add their rows n = g, g + 16, ... in index order, the 16
// partial sums meet in LDS and are added in group order.  One launch, no atomics, the same bits on every call.
//
// cov_f64_kernel: one 64 x 64 output tile per 4-wave block, only the T (T + 1) / 2 tiles on and above the diagonal (T = ceil(D / 64):
// 528 blocks at D = 2048, more than the chip has CUs, so N is not split and nothing is handed from block to block).  Per chunk of 32
// rows the block centres its two 64-column panels in fp64 and stages them in LDS once ([k][column], row stride 80 doubles: the 16
// lanes of k and the 16 lanes of k + 1 then fall on opposite halves of the 64 banks); both operands of v_mfma_f64_16x16x4_f64 are read
// from that image -- A[i][k] and B[k][j] are both "row k, column i or j" of it, lane l holding k = l >> 4, column l & 15 -- and a
// diagonal tile stages one panel only.  A wave owns a 32 x 32 quarter as 2 x 2 MFMA tiles; the next chunk's global loads are issued
// before the current chunk's MFMAs.  The sum over n runs in index order in every accumulator, rows past N and columns past D enter
// as zeros.  C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 map.  The epilogue divides by
// N - 1 (a division, one rounding) and writes each element and its mirror image from the same register: cov is bitwise symmetric
// by construction, also inside a diagonal tile (elements below the diagonal are written by their mirror only).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 256;        // 4 wave64
constexpr int MC = 16;         // columns per block of the mean kernel (and its row groups: MC * MC = NT)
constexpr int CT = 64;         // output tile edge of the covariance kernel
constexpr int KC = 32;         // rows of x per staged chunk (8 MFMA k-steps of 4)
constexpr int LDW = 80;        // LDS row stride in doubles (64 columns + 16: 160 dwords = 32 banks mod 64)
constexpr int RPT = KC * CT / NT;   // staged elements per thread and panel
constexpr long long N_MAX = 2147483647LL;
constexpr int D_MAX = 65536;

typedef double f64x4 __attribute__((ext_vector_type(4)));

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

__global__ __launch_bounds__(NT) void col_mean_f64_kernel(const float* __restrict__ x, long long N, int D, double* __restrict__ mean) {
    __shared__ double part[MC][MC + 1];
    const int c = threadIdx.x & (MC - 1), g = threadIdx.x / MC;
    const int col = blockIdx.x * MC + c;
    double s = 0.0;
    if (col < D) {
        const float* xc = x + col;
        long long n = g;
        for (; n + 3 * MC < N; n += 4 * MC) {                 // four loads in flight, added in index order
            const float v0 = xc[(size_t)n * D], v1 = xc[(size_t)(n + MC) * D], v2 = xc[(size_t)(n + 2 * MC) * D],
                        v3 = xc[(size_t)(n + 3 * MC) * D];
            s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
        }
        for (; n < N; n += MC) s += (double)xc[(size_t)n * D];
    }
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && col < D) {
        double t = part[0][c];
#pragma unroll
        for (int k = 1; k < MC; ++k) t += part[k][c];
        mean[col] = t / (double)N;
    }
}

__global__ __launch_bounds__(NT) void cov_f64_kernel(const float* __restrict__ x, const double* __restrict__ mean, long long N, int D,
                                                     int T, double* __restrict__ cov) {
    __shared__ double sm[2][KC][LDW];
    // blockIdx.x counts the tiles of the upper triangle row by row: (0,0) .. (0,T-1), (1,1) .. (1,T-1), ...
    int bi = 0, rem = blockIdx.x;
    while (rem >= T - bi) { rem -= T - bi; ++bi; }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // staging: thread -> column tid & 63 of both panels, rows (tid >> 6) + 4 r of the chunk
    const int scol = tid & 63, srow = tid >> 6;
    const int ca = bi * CT + scol, cb = bj * CT + scol;
    const bool va = ca < D, vb = !diag && cb < D;
    const double ma = va ? mean[ca] : 0.0, mb = vb ? mean[cb] : 0.0;
    const float* xa = x + (va ? ca : 0);
    const float* xb = x + (vb ? cb : 0);
    float ra[RPT], rb[RPT];
    auto fetch = [&](long long n0) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const long long n = n0 + srow + 4 * r;
            const bool in = n < N;
            ra[r] = (va && in) ? xa[(size_t)n * D] : 0.f;
            rb[r] = (vb && in) ? xb[(size_t)n * D] : 0.f;
        }
    };
    auto stash = [&](long long n0) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const bool in = n0 + srow + 4 * r < N;
            sm[0][srow + 4 * r][scol] = (va && in) ? (double)ra[r] - ma : 0.0;
            if (!diag) sm[1][srow + 4 * r][scol] = (vb && in) ? (double)rb[r] - mb : 0.0;
        }
    };

    // compute: wave -> quarter (wr, wc) of the tile; lane -> k = lane >> 4 of a k-step, column lane & 15 of an MFMA tile
    const int wr = wave >> 1, wc = wave & 1, lk = lane >> 4, lc = lane & 15;
    const double* pa = &sm[0][lk][wr * 32 + lc];
    const double* pb = &sm[diag ? 0 : 1][lk][wc * 32 + lc];
    f64x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};

    fetch(0);
    for (long long n0 = 0; n0 < N; n0 += KC) {
        stash(n0);
        __syncthreads();
        if (n0 + KC < N) fetch(n0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a0 = pa[kk * 4 * LDW], a1 = pa[kk * 4 * LDW + 16];
            const double b0 = pb[kk * 4 * LDW], b1 = pb[kk * 4 * LDW + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    const double den = (double)(N - 1);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = bi * CT + wr * 32 + m * 16 + lk + 4 * j;       // f64 C/D map: row = (lane >> 4) + 4 * reg
                const int col = bj * CT + wc * 32 + n * 16 + lc;
                if (row >= D || col >= D || (diag && row > col)) continue;
                const double v = acc[m][n][j] / den;
                cov[(size_t)row * D + col] = v;
                if (row != col) cov[(size_t)col * D + row] = v;
            }
}

}  // namespace

extern "C" {

int mogan_col_mean_f64(const float* x, long long N, int D, double* mean, hipStream_t stream) {
    if (!x || !mean || N < 1 || D < 1 || N > N_MAX || D > D_MAX) return MOGAN_ERR_SHAPE;
    hipLaunchKernelGGL(col_mean_f64_kernel, dim3((D + MC - 1) / MC), dim3(NT), 0, stream, x, N, D, mean);
    return ok_launch();
}

int mogan_cov_f64(const float* x, const double* mean, long long N, int D, double* cov, hipStream_t stream) {
    if (!x || !mean || !cov || N < 2 || D < 1 || N > N_MAX || D > D_MAX) return MOGAN_ERR_SHAPE;
    const int T = (D + CT - 1) / CT;                          // <= 1024: T (T + 1) / 2 <= 524800 blocks
    hipLaunchKernelGGL(cov_f64_kernel, dim3(T * (T + 1) / 2), dim3(NT), 0, stream, x, mean, N, D, T, cov);
    return ok_launch();
}

}  // extern "C"
