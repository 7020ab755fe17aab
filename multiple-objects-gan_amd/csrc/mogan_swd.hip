// mogan_swd.hip -- the device side of the sliced Wasserstein distance of DESIGN.md section 9g (Karras et al. 2018, section 5): the
// Laplacian pyramid of a batch of images, the 7 x 7 neighbourhood descriptors gathered from a level, their per-channel moments, the
// projection of the standardised descriptors onto random directions and the sum of |sorted real - sorted fake| per direction.  The
// sort between the last two is torch.sort.  The reference repository has no code for this score.
//
// Pyramid.  w = (1, 4, 6, 4, 1) / 16 in both axes, indices mirrored WITHOUT repeating the edge sample (m(i, n) = -i below 0,
// 2 n - 2 - i from n on).  pyr_down_kernel: one thread per output pixel, five row sums of five taps, then the column sum.
// lap_residual_kernel: one thread per pixel of the finer level; the zero-inserted image is never formed -- a (mirrored) tap on an
// odd row or column contributes nothing, a tap on (2 y, 2 x) reads down[y][x]; the filter is the same one times 4.  Both kernels
// add the taps in index order; no contraction (the build has -ffp-contract=off), so the same inputs give the same bits.
//
// gather_kernel: a copy.  One thread per descriptor value, (channel, y, x) order inside a row; image and centre are clamped into
// the level so that a bad triple reads a wrong pixel and never another allocation (the host op checks what it uploads).
//
// moments: two passes, each a fixed partition of the rows into P = min(ceil(rows / 64), 2048) contiguous shares.  A block adds its
// share per channel in fp64 (a thread walks the share's values with stride 256 in index order, the 256 partial sums meet in a fixed
// LDS tree) and leaves C doubles in the workspace; a one-block launch adds the shares in share order.  Pass 1 gives the mean,
// pass 2 sum (x - mean)^2 and from it the population standard deviation.  No atomics.
//
// project_kernel: out[d][r] = sum_k z[r][k] dirs[k][d], z = float((double(v) - mean_c) / std_c).  A block owns 64 descriptor rows,
// which are ONE contiguous piece of memory: it reads them coalesced, standardises them once and keeps them in LDS with the K tail
// (K = 49 C is never a multiple of 16) zero-filled up to KP.  Its four waves are 2 (row halves of 32) x 2 (direction halves of 64)
// and walk the directions in passes of 128; per 16 values of k one mma_k16 of csrc/mogan_mma.h (the split-bf16 product on the
// matrix pipe, or the native fp32 MFMA under MOGAN_X6=0) into a FRESH fp32 accumulator, and the groups of 16 are added in fp64 in
// index order and rounded to fp32 once.  (One accumulator carried through all groups rounds each of the six partial products of
// every group at the magnitude of the running sum -- 24 roundings for K = 49, measured 1.7 ulp off on a single projection where
// numpy's fp32 dot product is 0.3 ulp off; from zero the five small partial products round at their own magnitude, 2^-8 of the
// group's, and only the last one at the group's.)  The descriptor row is the MFMA's B operand, so a lane's 16 results are
// 16 directions of one row and the 32 lanes of a half-wave store 128 contiguous bytes of a direction's column.  Rows past `rows`,
// directions past D and k past K enter as zeros and are never stored; every result is one dot product over k in index order in a
// column of the MFMA of its own, so its bits depend on its row and its direction only.
//
// absdiff_kernel: one 1024-thread block per direction; thread t adds |a - b| over the quads t, t + 1024, ... of its column in fp64,
// element by element in index order (16-byte loads where the column is aligned, the same order where it is not), then the fixed
// LDS tree.
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include "../../include/mogan_hip.h"
#include "mogan_mma.h"

namespace {

constexpr int NT = 256;
constexpr long long I31 = 2147483647LL;
constexpr int PATCH = 7, PP = PATCH * PATCH;   // 49 values per channel and descriptor
constexpr int C_MAX = 4;
constexpr int D_MAX = 1024;
constexpr int SHARE_ROWS = 64, SHARES_MAX = 2048;
constexpr int PR = 64, PD = 128;               // rows per block, directions per pass of project_kernel
constexpr int AT = 1024;                       // threads of absdiff_kernel

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float tap_w(int t) { return t == 2 ? 0.375f : ((t == 1 || t == 3) ? 0.25f : 0.0625f); }

__global__ __launch_bounds__(NT) void pyr_down_kernel(const float* __restrict__ x, long long total, int H, int W,
                                                      float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int OW = W >> 1, OH = H >> 1;
    const int ox = (int)(i % OW);
    const long long t = i / OW;
    const int oy = (int)(t % OH);
    const float* p = x + (size_t)(t / OH) * H * W;
    int xs[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) xs[d] = mirror(2 * ox + d - 2, W);
    float s = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const float* row = p + (size_t)mirror(2 * oy + dy - 2, H) * W;
        float r = 0.f;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) r += tap_w(dx) * row[xs[dx]];
        s += tap_w(dy) * r;
    }
    out[i] = s;
}

__global__ __launch_bounds__(NT) void lap_residual_kernel(const float* __restrict__ x, const float* __restrict__ down,
                                                          long long total, int H, int W, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int hw = W >> 1, hh = H >> 1;
    const int px = (int)(i % W);
    const long long t = i / W;
    const int py = (int)(t % H);
    const float* p = down + (size_t)(t / H) * hh * hw;
    int xs[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) xs[d] = mirror(px + d - 2, W);
    float s = 0.f;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const int zy = mirror(py + dy - 2, H);
        if (zy & 1) continue;                                       // a row of inserted zeros
        const float* row = p + (size_t)(zy >> 1) * hw;
        float r = 0.f;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx)
            if (!(xs[dx] & 1)) r += tap_w(dx) * row[xs[dx] >> 1];
        s += tap_w(dy) * r;
    }
    out[i] = x[i] - 4.f * s;
}

__global__ __launch_bounds__(NT) void gather_kernel(const float* __restrict__ lvl, int N, int C, int H, int W,
                                                    const int32_t* __restrict__ tri, long long total, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int K = C * PP;
    const long long r = i / K;
    const int k = (int)(i - r * K);
    const int c = k / PP, q = k - c * PP, dy = q / PATCH, dx = q - dy * PATCH;
    const int32_t* t = tri + (size_t)r * 3;
    const int img = min(max(t[0], 0), N - 1), cy = min(max(t[1], 3), H - 4), cx = min(max(t[2], 3), W - 4);
    out[i] = lvl[(((size_t)img * C + c) * H + (cy - 3 + dy)) * W + (cx - 3 + dx)];
}

__host__ __device__ static inline long long shares_of(long long rows) {
    const long long s = (rows + SHARE_ROWS - 1) / SHARE_ROWS;
    return s > SHARES_MAX ? SHARES_MAX : s;
}

// the 256 per-thread sums of a block, per channel, in a fixed tree; the result in red[c][0]
__device__ __forceinline__ void block_tree(double (&acc)[C_MAX], double (*red)[NT]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < C_MAX; ++c) red[c][tid] = acc[c];
    __syncthreads();
    for (int off = NT / 2; off >= 1; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int c = 0; c < C_MAX; ++c) red[c][tid] += red[c][tid + off];
        }
        __syncthreads();
    }
}

// PASS 0: part[share][c] = sum x; PASS 1: sum (x - mean_c)^2 with mean_c = mom[2 c]
template <int PASS>
__global__ __launch_bounds__(NT) void moments_part_kernel(const float* __restrict__ x, long long rows, int C,
                                                          const double* __restrict__ mom, double* __restrict__ part) {
    __shared__ double red[C_MAX][NT];
    const int K = C * PP;
    const long long P = gridDim.x;
    const long long r_lo = rows * blockIdx.x / P, r_hi = rows * (blockIdx.x + 1) / P;
    const size_t e_lo = (size_t)r_lo * K, e_hi = (size_t)r_hi * K;
    double mean[C_MAX];
#pragma unroll
    for (int c = 0; c < C_MAX; ++c) mean[c] = (PASS == 1 && c < C) ? mom[2 * c] : 0.0;
    double acc[C_MAX] = {0.0, 0.0, 0.0, 0.0};
    int k = (int)((e_lo + threadIdx.x) % (size_t)K);                // the position inside the row, carried along
    for (size_t e = e_lo + threadIdx.x; e < e_hi; e += NT) {
        const int c = k / PP;
        k += NT % K;
        k -= k >= K ? K : 0;
        const double v = (double)x[e];
#pragma unroll
        for (int j = 0; j < C_MAX; ++j)
            if (j == c) {
                if (PASS == 0) {
                    acc[j] += v;
                } else {
                    const double d = v - mean[j];
                    acc[j] += d * d;
                }
            }
    }
    block_tree(acc, red);
    if (threadIdx.x < C) part[(size_t)blockIdx.x * C + threadIdx.x] = red[threadIdx.x][0];
}

// one block: the shares in share order.  PASS 0: mom[2 c] = sum / n; PASS 1: mom[2 c + 1] = sqrt(sum / n)
template <int PASS>
__global__ __launch_bounds__(64) void moments_finish_kernel(const double* __restrict__ part, long long P, int C, long long rows,
                                                            double* __restrict__ mom) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (long long b = 0; b < P; ++b) s += part[(size_t)b * C + c];
    const double n = (double)rows * (double)PP;
    if (PASS == 0) mom[2 * c] = s / n;
    else mom[2 * c + 1] = sqrt(s / n);
}

__global__ __launch_bounds__(NT) void project_kernel(const float* __restrict__ desc, long long rows, int C, int KP,
                                                     const double* __restrict__ mom, const float* __restrict__ dirs, int D,
                                                     float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sb[];      // [PR][KP + 4]: the standardised rows, k tail zero;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;  // behind them the 2 C moments (all LDS is dynamic)
    const int K = C * PP, LDB = KP + 4;
    double* sm = (double*)(sb + PR * LDB);
    const long long r0 = (long long)blockIdx.x * PR;
    const int nr = (int)(rows - r0 < PR ? rows - r0 : PR);
    if (tid < 2 * C) sm[tid] = mom[tid];
    __syncthreads();
    const float* src = desc + (size_t)r0 * K;
    for (int e = tid; e < PR * K; e += NT) {
        const int r = e / K, k = e - r * K;
        float z = 0.f;
        if (r < nr) {
            const int c = k / PP;
            z = (float)(((double)src[e] - sm[2 * c]) / sm[2 * c + 1]);
        }
        sb[r * LDB + k] = z;
    }
    const int tail = KP - K;
    for (int e = tid; e < PR * tail; e += NT) {
        const int r = e / tail;
        sb[r * LDB + K + (e - r * tail)] = 0.f;
    }
    __syncthreads();
    const int wr = wave & 1, wd = wave >> 1, l31 = lane & 31, h = lane >> 5;
    const float* brow = sb + (wr * 32 + l31) * LDB + h * 8;
    const long long row = r0 + wr * 32 + l31;
    for (int d0 = 0; d0 < D; d0 += PD) {
        double sum[2][16];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) sum[t][r] = 0.0;
        const int da = d0 + wd * 64 + l31;
        for (int g = 0; g < KP / 16; ++g) {
            float a[2][8], b[1][8];
            mma_f32x16 acc[2][1];                                   // a fresh accumulator per 16 values of k: see the header
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][0][r] = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = g * 16 + h * 8 + i;
                b[0][i] = brow[g * 16 + i];
#pragma unroll
                for (int t = 0; t < 2; ++t) a[t][i] = (k < K && da + t * 32 < D) ? dirs[(size_t)k * D + da + t * 32] : 0.f;
            }
            mma_k16<2, 1>(a, b, acc);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) sum[t][r] += (double)acc[t][0][r];
        }
        if (row < rows) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int d = d0 + wd * 64 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (d < D) out[(size_t)d * (size_t)rows + (size_t)row] = (float)sum[t][r];
                }
        }
    }
}

__global__ __launch_bounds__(AT) void absdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, long long rows,
                                                     double* __restrict__ out) {
    __shared__ double red[AT];
    const int tid = threadIdx.x;
    const float* pa = a + (size_t)blockIdx.x * (size_t)rows;
    const float* pb = b + (size_t)blockIdx.x * (size_t)rows;
    const bool vec = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
    const long long quads = (rows + 3) >> 2;
    double acc = 0.0;
    for (long long q = tid; q < quads; q += AT) {
        const long long e = q << 2;
        float va[4], vb[4];
        if (vec && e + 4 <= rows) {
            const float4 fa = *(const float4*)(pa + e), fb = *(const float4*)(pb + e);
            va[0] = fa.x; va[1] = fa.y; va[2] = fa.z; va[3] = fa.w;
            vb[0] = fb.x; vb[1] = fb.y; vb[2] = fb.z; vb[3] = fb.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = e + j < rows;
                va[j] = in ? pa[e + j] : 0.f;
                vb[j] = in ? pb[e + j] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += fabs((double)va[j] - (double)vb[j]);
    }
    red[tid] = acc;
    __syncthreads();
    for (int off = AT / 2; off >= 1; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = red[0];
}

static inline bool plane_ok(long long NC, int H, int W) {
    if (NC < 1 || NC > I31 || H < 4 || W < 4 || (H & 1) || (W & 1)) return false;
    return (long long)H * (long long)W <= I31 / NC;                 // NC H W <= 2^31 - 1
}

static inline unsigned blocks_of(long long total) { return (unsigned)((total + NT - 1) / NT); }

}  // namespace

extern "C" {

int mogan_pyr_down(const float* x, long long NC, int H, int W, float* out, hipStream_t stream) {
    if (!x || !out || !plane_ok(NC, H, W)) return MOGAN_ERR_SHAPE;
    const long long total = NC * (H / 2) * (W / 2);
    hipLaunchKernelGGL(pyr_down_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, x, total, H, W, out);
    return ok_launch();
}

int mogan_lap_residual(const float* x, const float* down, long long NC, int H, int W, float* out, hipStream_t stream) {
    if (!x || !down || !out || out == x || out == down || !plane_ok(NC, H, W)) return MOGAN_ERR_SHAPE;
    const long long total = NC * H * W;
    hipLaunchKernelGGL(lap_residual_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, x, down, total, H, W, out);
    return ok_launch();
}

int mogan_swd_gather(const float* level, int N, int C, int H, int W, const int32_t* centres, long long R, float* desc,
                     long long row0, long long rows_total, hipStream_t stream) {
    if (!level || !centres || !desc || N < 1 || C < 1 || C > C_MAX || H < PATCH || W < PATCH) return MOGAN_ERR_SHAPE;
    if ((long long)H * W > I31 / ((long long)N * C)) return MOGAN_ERR_SHAPE;
    if (R < 1 || row0 < 0 || rows_total < 1 || rows_total > I31 || R > rows_total || row0 > rows_total - R) return MOGAN_ERR_SHAPE;
    const int K = C * PP;
    const long long total = R * K;
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_of(total)), dim3(NT), 0, stream, level, N, C, H, W, centres, total,
                       desc + (size_t)row0 * K);
    return ok_launch();
}

size_t mogan_swd_moments_ws_bytes(long long rows, int C) {
    if (rows < 1 || rows > I31 || C < 1 || C > C_MAX) return 0;
    return (size_t)shares_of(rows) * (size_t)C * sizeof(double);
}

int mogan_swd_moments_f64(const float* desc, long long rows, int C, double* moments, void* ws, size_t ws_bytes,
                          hipStream_t stream) {
    if (!desc || !moments || rows < 1 || rows > I31 || C < 1 || C > C_MAX) return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_swd_moments_ws_bytes(rows, C)) return MOGAN_ERR_WS;
    const long long P = shares_of(rows);
    double* part = (double*)ws;
    hipLaunchKernelGGL(moments_part_kernel<0>, dim3((unsigned)P), dim3(NT), 0, stream, desc, rows, C, (const double*)moments, part);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(moments_finish_kernel<0>, dim3(1), dim3(64), 0, stream, (const double*)part, P, C, rows, moments);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(moments_part_kernel<1>, dim3((unsigned)P), dim3(NT), 0, stream, desc, rows, C, (const double*)moments, part);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(moments_finish_kernel<1>, dim3(1), dim3(64), 0, stream, (const double*)part, P, C, rows, moments);
    return ok_launch();
}

int mogan_swd_project(const float* desc, long long rows, int C, const double* moments, const float* dirs, int D, float* out,
                      hipStream_t stream) {
    if (!desc || !moments || !dirs || !out || rows < 1 || rows > I31 || C < 1 || C > C_MAX || D < 1 || D > D_MAX)
        return MOGAN_ERR_SHAPE;
    const int K = C * PP, KP = (K + 15) / 16 * 16;
    const size_t lds = (size_t)PR * (KP + 4) * sizeof(float) + 2 * C_MAX * sizeof(double);
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((rows + PR - 1) / PR)), dim3(NT), lds, stream, desc, rows, C, KP, moments,
                       dirs, D, out);
    return ok_launch();
}

int mogan_swd_absdiff_f64(const float* a, const float* b, long long rows, int D, double* out, hipStream_t stream) {
    if (!a || !b || !out || rows < 1 || rows > I31 || D < 1 || D > D_MAX) return MOGAN_ERR_SHAPE;
    hipLaunchKernelGGL(absdiff_kernel, dim3((unsigned)D), dim3(AT), 0, stream, a, b, rows, out);
    return ok_launch();
}

}  // extern "C"
