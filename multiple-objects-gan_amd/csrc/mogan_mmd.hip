// mogan_mmd.hip -- the sums the kernel Inception distance of DESIGN.md section 9e is computed from: for S subset pairs of s rows of
// x (Nx, D) and s rows of y (Ny, D), gathered through ix[k][:] and iy[k][:], under the polynomial kernel
//
//   k(a, b)    = (gamma <a, b> + coef0)^3
//   sums[k][0] = sum_{i != j} k(x_ix[k][i], x_ix[k][j])        ordered pairs, i != j by POSITION in the subset
//   sums[k][1] = sum_{i != j} k(y_iy[k][i], y_iy[k][j])
//   sums[k][2] = sum_{i, j}   k(x_ix[k][i], y_iy[k][j])
//
// x and y are fp32, widened exactly; everything after the load is fp64.  The reference repository has no code for this.
//
// poly3_mmd_kernel: one 64 x 64 tile of one subset's kernel matrix per 4-wave block and none of the matrix ever written.  Grid
// (tile, subset), the tile index fastest -- one subset's rows are in flight together.  Per subset the tiles are counted as: the
// P = T (T + 1) / 2 tiles on and above the diagonal of xx row by row, the same P of yy, then all T^2 of xy row by row
// (T = ceil(s / 64): 528 tiles at s = 1000).  The tile of <a_i, b_j> is gram64_tile of csrc/mogan_gram64.h on two row panels of
// GATHERED rows: the reduction runs along the feature axis in index order in every accumulator; rows past s and features past D
// enter as zeros.  An index outside [0, N) is clamped, so a bad device index cannot read outside x or y.
//
// Epilogue.  t = acc * gamma + coef0, value (t * t) * t, no contraction.  A zero row is not a zero kernel value (k = coef0^3), so
// rows and columns past s are masked out of the sum again; a diagonal tile of xx / yy keeps i < j only.  A lane adds its 16 masked
// values in register order, the wave reduces in a fixed butterfly (xor 32, 16, 8, 4, 2, 1), the four waves meet in LDS and are
// added in wave order; tiles of xx / yy are doubled (exact) and the block writes ONE double to ws[subset][tile].  No atomics.
//
// poly3_mmd_finish_kernel: one block per subset, three threads; thread q adds the tile partials of sum q in tile order.  A
// subset's three sums depend on nothing but that subset's rows, and the same inputs give the same bits on every call.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mogan_gram64.h"

namespace {

constexpr int S_MAX = 65535;                 // grid.y
constexpr int SUB_MAX = 1 << 20;             // T <= 16384: 2 T^2 + T tiles stay below 2^31

static inline long long tiles_of(int s) {
    const long long T = (s + CT - 1) / CT;
    return T * (T + 1) + T * T;
}

template <bool VEC>
__global__ __launch_bounds__(NT) void poly3_mmd_kernel(const float* __restrict__ x, long long Nx, const float* __restrict__ y,
                                                       long long Ny, int D, const int32_t* __restrict__ ix,
                                                       const int32_t* __restrict__ iy, int s, int T, double gamma, double coef0,
                                                       double* __restrict__ ws) {
    __shared__ GramLds sm;
    __shared__ double red[NT / 64];
    const int P = T * (T + 1) / 2;
    const int tile = blockIdx.x, subset = blockIdx.y;
    // kind 0 = xx, 1 = yy (upper triangle, row by row), 2 = xy (all tiles, row by row)
    int kind, bi, bj;
    if (tile < 2 * P) {
        kind = tile >= P ? 1 : 0;
        gram_upper_tile(tile - kind * P, T, bi, bj);
    } else {
        kind = 2;
        const int r = tile - 2 * P;
        bi = r / T;
        bj = r - bi * T;
    }
    const bool sym = kind != 2, diag = sym && bi == bj;
    const float* A = kind == 1 ? y : x;
    const float* B = kind == 0 ? x : y;
    const long long NA = kind == 1 ? Ny : Nx, NB = kind == 0 ? Nx : Ny;
    const int32_t* ia = (kind == 1 ? iy : ix) + (size_t)subset * s;
    const int32_t* ib = (kind == 0 ? ix : iy) + (size_t)subset * s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // the staged rows of this thread: subset positions pa, pb -> gathered, clamped rows of A and B
    const int pa = bi * CT + RowPanels<VEC>::stage_row(), pb = bj * CT + RowPanels<VEC>::stage_row();
    const bool va = pa < s, vb = !diag && pb < s;
    long long ra_i = va ? (long long)ia[pa] : 0, rb_i = vb ? (long long)ib[pb] : 0;
    ra_i = ra_i < 0 ? 0 : (ra_i > NA - 1 ? NA - 1 : ra_i);
    rb_i = rb_i < 0 ? 0 : (rb_i > NB - 1 ? NB - 1 : rb_i);
    RowPanels<VEC> src(A + (size_t)ra_i * D, va, B + (size_t)rb_i * D, vb, D, diag);
    f64x4 acc[2][2];
    gram64_tile(src, sm, acc);

    const GramLane ln;
    double part = 0.0;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = ln.row(bi * CT, m, j), col = ln.col(bj * CT, n);
                    const bool keep = row < s && col < s && (!diag || row < col);
                    const double t = acc[m][n][j] * gamma + coef0;
                    const double v = (t * t) * t;
                    part += keep ? v : 0.0;
                }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) t += red[w];
        ws[(size_t)subset * gridDim.x + tile] = sym ? t + t : t;
    }
}

__global__ __launch_bounds__(64) void poly3_mmd_finish_kernel(const double* __restrict__ ws, int ntiles, int P,
                                                              double* __restrict__ sums) {
    const int q = threadIdx.x;
    if (q >= 3) return;
    const double* w = ws + (size_t)blockIdx.x * ntiles;
    const int lo = q * P, hi = q == 2 ? ntiles : (q + 1) * P;
    double t = 0.0;
    for (int i = lo; i < hi; ++i) t += w[i];
    sums[(size_t)blockIdx.x * 3 + q] = t;
}

}  // namespace

extern "C" {

size_t mogan_poly3_mmd_ws_bytes(int S, int s) {
    if (S < 1 || s < 2 || S > S_MAX || s > SUB_MAX) return 0;
    return (size_t)S * (size_t)tiles_of(s) * sizeof(double);
}

int mogan_poly3_mmd_f64(const float* x, long long Nx, const float* y, long long Ny, int D, const int32_t* ix, const int32_t* iy,
                        int S, int s, double gamma, double coef0, double* sums, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!x || !y || !ix || !iy || !sums || S < 1 || s < 2 || D < 1 || Nx < 1 || Ny < 1 || D > D_MAX || S > S_MAX || s > SUB_MAX ||
        Nx > N_MAX || Ny > N_MAX || !std::isfinite(gamma) || !std::isfinite(coef0))
        return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_poly3_mmd_ws_bytes(S, s)) return MOGAN_ERR_WS;
    const int T = (s + CT - 1) / CT;
    const int ntiles = (int)tiles_of(s);
    const bool vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
    const dim3 grid(ntiles, S);
    if (vec)
        hipLaunchKernelGGL(poly3_mmd_kernel<true>, grid, dim3(NT), 0, stream, x, Nx, y, Ny, D, ix, iy, s, T, gamma, coef0,
                           (double*)ws);
    else
        hipLaunchKernelGGL(poly3_mmd_kernel<false>, grid, dim3(NT), 0, stream, x, Nx, y, Ny, D, ix, iy, s, T, gamma, coef0,
                           (double*)ws);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(poly3_mmd_finish_kernel, dim3(S), dim3(64), 0, stream, (const double*)ws, ntiles, T * (T + 1) / 2,
                       sums);
    return ok_launch();
}

}  // extern "C"
