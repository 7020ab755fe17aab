// mogan_spectrum.hip -- the device side of the radial power spectrum of DESIGN.md section 9k (the azimuthally averaged power
// spectrum of Durall et al. 2020, Dzanic et al. 2020 and Schwarz et al. 2021): per image, the sum of |F[u, v]|^2 over the members of
// every bin of a host-built table, F the unnormalised 2-D DFT of the windowed luminance plane.  attngan/spectrum.py holds the
// definition; the reference repository has no code for it.  Everything after the fp32 loads is fp64; the twiddle factors come from
// a host table, the device calls no trigonometric function.
//
// Every block of every launch works on ONE image, and an image's arithmetic does not depend on where in the batch it stands or on
// how large the batch is: row b of the output has the bits it has at B = 1.  A call walks the batch in chunks of at most CHUNK
// images, so the workspace is bounded by min(B, CHUNK) images whatever B is.
//
// spectrum_rows_kernel: a block owns ROWS = min(S, 2048 / S) rows of one image.  On load a pixel becomes
//     y = sum_c (double) weight[c] * (double) x[c]   (c ascending),   y * ((double) window[i] * (double) window[j])
// and goes to its bit-reversed place in LDS; log2 S in-place radix-2 stages (decimation in time) follow, a barrier after each; the
// S / 2 + 1 non-negative frequencies of every row go to the workspace as G[v][i], so that a column is contiguous for the next launch.
// spectrum_cols_kernel: a block owns COLS = min(S / 2 + 1, 2048 / S) columns v of one image: the same transform along i, then
// m(v) (re^2 + im^2) with m = 1 for v in {0, S / 2} and 2 otherwise in place of the real part, the columns' slice of the bin table
// next to it in LDS, and thread k < n_bins adds the members of bin k in (column, u) order -- any table is legal, nothing is assumed
// about where a bin's members lie.  The block leaves n_bins partial sums in the workspace.  No 2-D power plane reaches memory.
// spectrum_finish_kernel: thread (image, k) adds the image's column groups in index order.  No atomics anywhere.
// A zero image gives +0.0 in every stage, and so exactly 0.0 in every bin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 256;
constexpr int ELEMS = 2048;                    // complex doubles a block transforms in LDS (32 KB)
constexpr int S_MIN = 8, S_MAX = 256;
constexpr int C_MAX = 4;
constexpr int BINS_MAX = 256;                  // one thread per bin
constexpr int CHUNK = 64;                      // images per round of the three launches
constexpr long long I31 = 2147483647LL;

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

static inline bool size_ok(int S) { return S >= S_MIN && S <= S_MAX && (S & (S - 1)) == 0; }
static inline int rows_of(int S) { return S < ELEMS / S ? S : ELEMS / S; }                       // rows per block, first launch
static inline int cols_of(int S) { return S / 2 + 1 < ELEMS / S ? S / 2 + 1 : ELEMS / S; }       // columns per block, second launch
static inline int groups_of(int S) { return (S / 2 + 1 + cols_of(S) - 1) / cols_of(S); }
static inline size_t half_bytes(int S) { return (size_t)(S / 2 + 1) * (size_t)S * sizeof(double2); }
static inline size_t image_bytes(int S) { return half_bytes(S) + (size_t)groups_of(S) * BINS_MAX * sizeof(double); }

// `lines` transforms of length S = 2^log2S side by side in a[line * S + .], input in bit-reversed order; tw[k] = (cos, -sin)(2 pi k / S)
__device__ __forceinline__ void fft_lines(double2* a, const double2* tw, int lines, int S, int log2S) {
    const int half = S >> 1, total = lines * half;
    for (int s = 0; s < log2S; ++s) {
        const int m = 1 << s;                                       // half the butterfly span
        __syncthreads();
        for (int e = threadIdx.x; e < total; e += NT) {
            const int line = e / half, t = e - line * half;
            const int j = t & (m - 1);
            const int pos = line * S + ((t - j) << 1) + j;
            const double2 w = tw[j << (log2S - 1 - s)];
            const double2 lo = a[pos], hi = a[pos + m];
            const double xr = hi.x * w.x - hi.y * w.y, xi = hi.x * w.y + hi.y * w.x;
            a[pos] = make_double2(lo.x + xr, lo.y + xi);
            a[pos + m] = make_double2(lo.x - xr, lo.y - xi);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int bit_reverse(int i, int log2S) { return (int)(__brev((unsigned)i) >> (32 - log2S)); }

__global__ __launch_bounds__(NT) void spectrum_rows_kernel(const float* __restrict__ x, int C, int S, int log2S, int rows,
                                                           const float* __restrict__ weight, const float* __restrict__ window,
                                                           const double2* __restrict__ twiddle, double2* __restrict__ G) {
    __shared__ double2 a[ELEMS];
    __shared__ double2 tw[S_MAX / 2];
    __shared__ double sw[S_MAX];
    __shared__ double wc[C_MAX];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * rows;
    const size_t plane = (size_t)S * S;
    const float* img = x + (size_t)blockIdx.y * C * plane;
    double2* g = G + (size_t)blockIdx.y * (size_t)(S / 2 + 1) * S;
    if (tid < S / 2) tw[tid] = twiddle[tid];
    if (tid < S) sw[tid] = window ? (double)window[tid] : 1.0;
    if (tid < C) wc[tid] = (double)weight[tid];
    __syncthreads();
    for (int e = tid; e < rows * S; e += NT) {
        const int r = e / S, j = e - r * S;
        const size_t at = (size_t)(i0 + r) * S + j;
        double y = 0.0;
        for (int c = 0; c < C; ++c) y += wc[c] * (double)img[c * plane + at];
        if (window) y = y * (sw[i0 + r] * sw[j]);
        a[r * S + bit_reverse(j, log2S)] = make_double2(y, 0.0);
    }
    fft_lines(a, tw, rows, S, log2S);
    for (int e = tid; e < (S / 2 + 1) * rows; e += NT) {
        const int v = e / rows, r = e - v * rows;
        g[(size_t)v * S + i0 + r] = a[r * S + v];
    }
}

__global__ __launch_bounds__(NT) void spectrum_cols_kernel(const double2* __restrict__ G, int S, int log2S, int cols, int groups,
                                                           const double2* __restrict__ twiddle, const int* __restrict__ bins,
                                                           int n_bins, double* __restrict__ part) {
    __shared__ double2 a[ELEMS];
    __shared__ double2 tw[S_MAX / 2];
    __shared__ int sb[ELEMS];
    const int tid = threadIdx.x;
    const int V = S / 2 + 1;
    const int v0 = blockIdx.x * cols;
    const int cb = V - v0 < cols ? V - v0 : cols;                   // this block's columns (the last group may hold fewer)
    const double2* g = G + (size_t)blockIdx.y * (size_t)V * S + (size_t)v0 * S;
    if (tid < S / 2) tw[tid] = twiddle[tid];
    for (int e = tid; e < cb * S; e += NT) {
        const int c = e / S, i = e - c * S;
        a[c * S + bit_reverse(i, log2S)] = g[e];
        sb[e] = bins[(size_t)i * V + v0 + c];                       // sb[c][u]: the table's (u, v0 + c)
    }
    fft_lines(a, tw, cb, S, log2S);
    for (int e = tid; e < cb * S; e += NT) {
        const int v = v0 + e / S;
        const double2 z = a[e];
        const double p = z.x * z.x + z.y * z.y;
        a[e].x = (v == 0 || v == S / 2) ? p : 2.0 * p;
    }
    __syncthreads();
    if (tid < n_bins) {
        double acc = 0.0;
        const int total = cb * S;
        // x + 0.0 = x bit for bit for the sums of squares here (never -0.0): the select keeps the loop free of branches, so its LDS
        // reads -- broadcasts, every thread reads the same address -- can be issued ahead of the adds, which stay in (column, u) order
#pragma unroll 8
        for (int e = 0; e < total; ++e) acc += (sb[e] == tid) ? a[e].x : 0.0;
        part[((size_t)blockIdx.y * groups + blockIdx.x) * n_bins + tid] = acc;
    }
}

__global__ __launch_bounds__(NT) void spectrum_finish_kernel(const double* __restrict__ part, int images, int groups, int n_bins,
                                                             double* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= images * n_bins) return;
    const int b = i / n_bins, k = i - b * n_bins;
    const double* src = part + (size_t)b * groups * n_bins + k;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += src[(size_t)g * n_bins];
    out[i] = s;
}

}  // namespace

extern "C" {

size_t mogan_radial_power_ws_bytes(int B, int S) {
    if (B < 1 || !size_ok(S)) return 0;
    return (size_t)(B < CHUNK ? B : CHUNK) * image_bytes(S);
}

int mogan_radial_power_f64(const float* x, int B, int C, int S, const float* weight, const float* window, const double* twiddle,
                           const int* bins, int n_bins, double* out, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!x || !weight || !twiddle || !bins || !out || B < 1 || !size_ok(S) || C < 1 || C > C_MAX || n_bins < 1 || n_bins > BINS_MAX)
        return MOGAN_ERR_SHAPE;
    if (((uintptr_t)twiddle & 15) != 0 || ((uintptr_t)out & 7) != 0) return MOGAN_ERR_SHAPE;     // read as double2 / written as double
    if ((long long)S * S > I31 / ((long long)B * C)) return MOGAN_ERR_SHAPE;                     // B C S S <= 2^31 - 1
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < mogan_radial_power_ws_bytes(B, S)) return MOGAN_ERR_WS;
    int log2S = 0;
    while ((1 << log2S) < S) ++log2S;
    const int rows = rows_of(S), cols = cols_of(S), groups = groups_of(S);
    const int chunk = B < CHUNK ? B : CHUNK;
    double2* G = (double2*)ws;
    double* part = (double*)((char*)ws + (size_t)chunk * half_bytes(S));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int n = B - b0 < chunk ? B - b0 : chunk;
        hipLaunchKernelGGL(spectrum_rows_kernel, dim3(S / rows, n), dim3(NT), 0, stream, x + (size_t)b0 * C * S * S, C, S, log2S, rows,
                           weight, window, (const double2*)twiddle, G);
        if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
        hipLaunchKernelGGL(spectrum_cols_kernel, dim3(groups, n), dim3(NT), 0, stream, (const double2*)G, S, log2S, cols, groups,
                           (const double2*)twiddle, bins, n_bins, part);
        if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
        hipLaunchKernelGGL(spectrum_finish_kernel, dim3((n * n_bins + NT - 1) / NT), dim3(NT), 0, stream, (const double*)part, n,
                           groups, n_bins, out + (size_t)b0 * n_bins);
        if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    }
    return 0;
}

}  // extern "C"
