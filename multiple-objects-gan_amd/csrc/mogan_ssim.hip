// mogan_ssim.hip -- the device side of the multi-scale structural similarity of DESIGN.md section 9h (Wang, Simoncelli & Bovik 2003;
// the diversity score of Odena et al. 2017): the aligned 2 x 2 mean that leads from one scale to the next, and one scale's
// (mean ssim, mean cs) for P pairs of images.  attngan/msssim.py holds the definition; the reference repository has no code for it.
//
// avg_down2_kernel: one thread per output pixel, ((x00 + x01) + (x10 + x11)) * 0.25f.
//
// ssim_tile_kernel: a block owns TILE x TILE = 32 x 32 valid positions of one channel of one pair.  It stages the (TILE + n - 1)^2
// input pixels of BOTH images as centred values d = 127.5f x in LDS (what lies past the image enters as zero and only feeds
// positions that are never stored or summed), filters the five planes d_a, d_b, d_a d_a, d_b d_b, d_a d_b along x into LDS -- the
// products are formed here, per staged pixel -- and then along y in registers: thread (tx, g) owns column tx and the four rows
// 4 g .. 4 g + 3 of the tile and walks the 4 + n - 1 rows of the x-filtered planes they need once, adding row r into output j
// with weight win[r - j].  Both filters start from zero and add their taps in index order; the build has -ffp-contract=off.  The
// five filtered planes never reach memory.  Per position
//     cs = (2 s_ab + C2) / ((s_aa + s_bb) + C2),  l = (2 (mu_a mu_b) + C1) / ((mu_a mu_a + mu_b mu_b) + C1),  ssim = l cs
// with IEEE division: for bit-identical images s_ab = s_aa = s_bb and mu_a = mu_b bit for bit, 2 s = s + s exactly, so both
// quotients are x / x = 1.0f; and every expression is symmetric in a and b operation by operation (a product and a two-term sum
// commute), so exchanging the images changes no bit.  A thread adds its up to four values in fp64 in row order, the 256 sums meet
// in a fixed LDS tree, and the block leaves (sum ssim, sum cs) in ws[pair][channel][tile].
//
// ssim_finish_kernel: one thread per pair and term adds the pair's C T T partials in index order and divides by C M M.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

namespace {

constexpr int NT = 256;
constexpr long long I31 = 2147483647LL;
constexpr int C_MAX = 4;
constexpr int N_MAX = 11;                      // the longest window
constexpr int TILE = 32;                       // valid positions per block and axis
constexpr int IN = TILE + N_MAX - 1;           // staged pixels per axis
constexpr int ROWS_PER_THREAD = TILE * TILE / NT;

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

__global__ __launch_bounds__(NT) void avg_down2_kernel(const float* __restrict__ x, long long total, int H, int W,
                                                       float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int OW = W >> 1, OH = H >> 1;
    const int ox = (int)(i % OW);
    const long long t = i / OW;
    const int oy = (int)(t % OH);
    const float* p = x + ((size_t)(t / OH) * H + 2 * oy) * W + 2 * ox;
    out[i] = ((p[0] + p[1]) + (p[W] + p[W + 1])) * 0.25f;
}

__global__ __launch_bounds__(NT) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int C, int S,
                                                       const float* __restrict__ win, int n, int T, double* __restrict__ part,
                                                       float* __restrict__ ssim_map, float* __restrict__ cs_map) {
    __shared__ float sa[IN][IN + 1], sb[IN][IN + 1];               // the centred pixels of both images
    __shared__ float hp[5][IN][TILE];                              // the five planes filtered along x
    __shared__ float sw[N_MAX];
    __shared__ double red[2][NT];
    const int tid = threadIdx.x;
    const int M = S - n + 1, ext = TILE + n - 1;                   // valid positions per axis; staged pixels per axis
    const int tile = blockIdx.x % (T * T);
    const long long plane = blockIdx.x / (T * T);                  // pair * C + channel
    const int y0 = (tile / T) * TILE, x0 = (tile % T) * TILE;
    const float* pa = a + (size_t)plane * S * S;
    const float* pb = b + (size_t)plane * S * S;
    if (tid < n) sw[tid] = win[tid];
    for (int e = tid; e < ext * ext; e += NT) {
        const int r = e / ext, c = e - r * ext;
        const int y = y0 + r, x = x0 + c;
        const bool in = y < S && x < S;
        sa[r][c] = in ? 127.5f * pa[(size_t)y * S + x] : 0.f;
        sb[r][c] = in ? 127.5f * pb[(size_t)y * S + x] : 0.f;
    }
    __syncthreads();
    for (int e = tid; e < ext * TILE; e += NT) {
        const int r = e / TILE, c = e % TILE;
        float f[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < n; ++k) {
            const float w = sw[k], va = sa[r][c + k], vb = sb[r][c + k];
            f[0] += w * va;
            f[1] += w * vb;
            f[2] += w * (va * va);
            f[3] += w * (vb * vb);
            f[4] += w * (va * vb);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hp[q][r][c] = f[q];
    }
    __syncthreads();
    const int tx = tid % TILE, g = tid / TILE;
    float acc[ROWS_PER_THREAD][5];
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[j][q] = 0.f;
    for (int r = 0; r < ROWS_PER_THREAD + n - 1; ++r) {            // r and j are the same for a whole wave: no divergence
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hp[q][ROWS_PER_THREAD * g + r][tx];
#pragma unroll
        for (int j = 0; j < ROWS_PER_THREAD; ++j) {
            const int k = r - j;
            if (k >= 0 && k < n) {
                const float w = sw[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[j][q] += w * v[q];
            }
        }
    }
    const float C1 = 6.5025f, C2 = 58.5225f;
    double sum_ssim = 0.0, sum_cs = 0.0;
    const int ox = x0 + tx;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
        const int oy = y0 + ROWS_PER_THREAD * g + j;
        if (oy < M && ox < M) {
            const float ma = acc[j][0], mb = acc[j][1];
            const float saa = acc[j][2] - ma * ma, sbb = acc[j][3] - mb * mb, sab = acc[j][4] - ma * mb;
            const float mua = 127.5f + ma, mub = 127.5f + mb;
            const float cs = (2.f * sab + C2) / ((saa + sbb) + C2);
            const float l = (2.f * (mua * mub) + C1) / ((mua * mua + mub * mub) + C1);
            const float ssim = l * cs;
            const size_t o = ((size_t)plane * M + oy) * M + ox;
            if (ssim_map) ssim_map[o] = ssim;
            if (cs_map) cs_map[o] = cs;
            sum_ssim += (double)ssim;
            sum_cs += (double)cs;
        }
    }
    red[0][tid] = sum_ssim;
    red[1][tid] = sum_cs;
    __syncthreads();
    for (int off = NT / 2; off >= 1; off >>= 1) {
        if (tid < off) {
            red[0][tid] += red[0][tid + off];
            red[1][tid] += red[1][tid + off];
        }
        __syncthreads();
    }
    if (tid < 2) part[(size_t)blockIdx.x * 2 + tid] = red[tid][0];
}

// terms[p][t] = (sum of pair p's `per_pair` partials of term t, in index order) / count
__global__ __launch_bounds__(64) void ssim_finish_kernel(const double* __restrict__ part, long long P, int per_pair, double count,
                                                         double* __restrict__ terms) {
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * P) return;
    const long long p = i >> 1;
    const int t = (int)(i & 1);
    const double* src = part + ((size_t)p * per_pair) * 2 + t;
    double s = 0.0;
    for (int k = 0; k < per_pair; ++k) s += src[(size_t)k * 2];
    terms[i] = s / count;
}

static inline bool level_ok(long long P, int C, int S, int n) {
    if (P < 1 || P > I31 || C < 1 || C > C_MAX || S < 2 || n < 1 || n > N_MAX || n > S) return false;
    return (long long)S * (long long)S <= I31 / (P * C);           // P C S S <= 2^31 - 1
}

static inline int tiles_of(int S, int n) { return (S - n + 1 + TILE - 1) / TILE; }

}  // namespace

extern "C" {

int mogan_avg_down2(const float* x, long long NC, int H, int W, float* out, hipStream_t stream) {
    if (!x || !out || NC < 1 || NC > I31 || H < 2 || W < 2 || (H & 1) || (W & 1)) return MOGAN_ERR_SHAPE;
    if ((long long)H * (long long)W > I31 / NC) return MOGAN_ERR_SHAPE;
    const long long total = NC * (H / 2) * (W / 2);
    hipLaunchKernelGGL(avg_down2_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, x, total, H, W, out);
    return ok_launch();
}

size_t mogan_ssim_level_ws_bytes(long long P, int C, int S, int n) {
    if (!level_ok(P, C, S, n)) return 0;
    const size_t T = (size_t)tiles_of(S, n);
    return (size_t)P * (size_t)C * T * T * 2 * sizeof(double);
}

int mogan_ssim_level_f64(const float* a, const float* b, long long P, int C, int S, const float* win, int n, double* terms,
                         float* ssim_map, float* cs_map, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!a || !b || !win || !terms || !level_ok(P, C, S, n)) return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_ssim_level_ws_bytes(P, C, S, n)) return MOGAN_ERR_WS;
    const int T = tiles_of(S, n), M = S - n + 1;
    const long long blocks = P * C * T * T;                        // <= P C S S <= 2^31 - 1
    double* part = (double*)ws;
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)blocks), dim3(NT), 0, stream, a, b, C, S, win, n, T, part, ssim_map, cs_map);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(64), 0, stream, (const double*)part, P,
                       C * T * T, (double)C * (double)M * (double)M, terms);
    return ok_launch();
}

}  // extern "C"
