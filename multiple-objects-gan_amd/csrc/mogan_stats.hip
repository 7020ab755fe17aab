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
// 528 blocks at D = 2048, more than the chip has CUs, so N is not split and nothing is handed from block to block).  The tile is
// gram64_tile of csrc/mogan_gram64.h on two centred column panels: the sum over n runs in index order in every accumulator, rows
// past N and columns past D enter as zeros.  The epilogue divides by N - 1 (a division, one rounding) and writes each element
// and its mirror image from the same register: cov is bitwise symmetric by construction, also inside a diagonal tile (elements
// below the diagonal are written by their mirror only).
#include <hip/hip_runtime.h>
#include "mogan_gram64.h"

namespace {

constexpr int MC = 16;         // columns per block of the mean kernel (and its row groups: MC * MC = NT)

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
    __shared__ GramLds sm;
    int bi, bj;
    gram_upper_tile(blockIdx.x, T, bi, bj);
    const bool diag = bi == bj;
    ColPanels src(x, mean, N, D, bi * CT, bj * CT, diag);
    f64x4 acc[2][2];
    gram64_tile(src, sm, acc);

    const GramLane ln;
    const double den = (double)(N - 1);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = ln.row(bi * CT, m, j), col = ln.col(bj * CT, n);
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
