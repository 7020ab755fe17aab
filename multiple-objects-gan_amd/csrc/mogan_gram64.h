// mogan_gram64.h -- one 64 x 64 tile of an fp64 Gram matrix on v_mfma_f64_16x16x4_f64, written once (internal, like mogan_mma.h
// and mogan_bn.h) for the evaluation kernels: cov_f64_kernel (mogan_stats.hip), poly3_mmd_kernel (mogan_mmd.hip), row_norm_kernel,
// knn_kernel, cross_kernel and ball_kernel (mogan_knn.hip).  They differ in where their two 64-wide panels come from and in what they do with
// the tile; the loop between is gram64_tile and nothing else.  DESIGN.md section 9d.
//
// acc[i][j] = sum_k a[k][i] b[k][j] for a 4-wave block.  Per chunk of KC = 32 values of k the block stages its two panels in LDS
// once, as [k][i] and [k][j] with a row stride of 80 doubles (64 + 16: 160 dwords = 32 banks mod 64, so the 16 lanes of k and the
// 16 lanes of k + 1 fall on opposite halves of the 64 banks); both MFMA operands are read from that image -- A[i][k] and B[k][j]
// are both "row k, column i or j" of it, lane l holding k = l >> 4, column l & 15 -- and a tile whose panels are the same (`same`:
// a diagonal tile) stages one panel only.  A wave owns a 32 x 32 quarter, (wave >> 1, wave & 1), as 2 x 2 MFMA tiles.  The next
// chunk's global loads are issued before the current chunk's MFMAs and wait in registers for the barrier behind them.
//
// What the callers' contracts rest on: every accumulator sees the K steps in index order; whatever lies past the end of a panel
// or of k enters as zero; the products of an MFMA commute.  So an element's bits depend on its two panel columns only -- not on
// the tile, the wave, or which operand a column is -- and acc[i][j] of (a, b) is bitwise acc[j][i] of (b, a).
//
// A panel source is a struct with index_t, extent, fetch(k0) (global -> registers) and stash(k0, sm) (registers -> the image):
//   RowPanels<VEC>  64 rows of an fp32 matrix each, k along the contiguous feature axis; the caller supplies each thread's row
//                   pointer and its validity, so a gathered row serves as well as base + row * D.
//   ColPanels       64 columns of x each minus their fp64 mean, k along the rows of x at stride D.
#ifndef MOGAN_GRAM64_H
#define MOGAN_GRAM64_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mogan_hip.h"

constexpr int NT = 256;        // 4 wave64
constexpr int CT = 64;         // tile edge
constexpr int KC = 32;         // values of k per staged chunk (8 MFMA k-steps of 4)
constexpr int LDW = 80;        // LDS row stride in doubles
constexpr int KPT = KC * CT / NT;   // staged elements per thread and panel
constexpr long long N_MAX = 2147483647LL;    // rows of a set (index tables are int32)
constexpr int D_MAX = 65536;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double GramLds[2][KC][LDW];          // the staging image: panel, k, column

static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

// A lane's place in the tile.  C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * reg -- NOT the f32 map.
// acc[m][n][j] is element (row(r0, m, j), col(c0, n)) of a matrix whose tile starts at (r0, c0), in the index type of r0, c0.
struct GramLane {
    int wr, wc, lk, lc;
    __device__ __forceinline__ GramLane() {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        wr = wave >> 1; wc = wave & 1; lk = lane >> 4; lc = lane & 15;
    }
    template <class I> __device__ __forceinline__ I row(I r0, int m, int j) const { return r0 + wr * 32 + m * 16 + lk + 4 * j; }
    template <class I> __device__ __forceinline__ I col(I c0, int n) const { return c0 + wc * 32 + n * 16 + lc; }
};

// tile index -> (bi, bj), the tiles of the upper triangle counted row by row: (0,0) .. (0,T-1), (1,1) .. (1,T-1), ...
__device__ __forceinline__ void gram_upper_tile(int rem, int T, int& bi, int& bj) {
    bi = 0;
    while (rem >= T - bi) { rem -= T - bi; ++bi; }
    bj = bi + rem;
}

// thread -> row tid >> 2 of both panels (stage_row(): the caller derives xa, xb from it), features (tid & 3) * 8 .. + 7 of the
// chunk: two 16-byte loads where VEC (D % 4 == 0 and 16-byte-aligned bases: a group of 4 features is inside D or past it), scalar
// loads otherwise.  Invalid rows and features past D enter as zeros; vb must be false where same.
template <bool VEC>
struct RowPanels {
    typedef int index_t;
    const float *xa, *xb;
    bool va, vb, same;
    int extent, srow, sk;
    float ra[KPT], rb[KPT];
    __device__ __forceinline__ static int stage_row() { return threadIdx.x >> 2; }
    __device__ __forceinline__ RowPanels(const float* xa_, bool va_, const float* xb_, bool vb_, int D, bool same_)
        : xa(xa_), xb(xb_), va(va_), vb(vb_), same(same_), extent(D), srow(stage_row()), sk((threadIdx.x & 3) * KPT) {}
    __device__ __forceinline__ void fetch(int k0) {
        if (VEC) {
#pragma unroll
            for (int h = 0; h < KPT / 4; ++h) {
                const int k = k0 + sk + 4 * h;
                const bool in = k < extent;
                const float4 a = (va && in) ? *reinterpret_cast<const float4*>(xa + k) : float4{0.f, 0.f, 0.f, 0.f};
                const float4 b = (vb && in) ? *reinterpret_cast<const float4*>(xb + k) : float4{0.f, 0.f, 0.f, 0.f};
                ra[4 * h] = a.x; ra[4 * h + 1] = a.y; ra[4 * h + 2] = a.z; ra[4 * h + 3] = a.w;
                rb[4 * h] = b.x; rb[4 * h + 1] = b.y; rb[4 * h + 2] = b.z; rb[4 * h + 3] = b.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < KPT; ++j) {
                const int k = k0 + sk + j;
                const bool in = k < extent;
                ra[j] = (va && in) ? xa[k] : 0.f;
                rb[j] = (vb && in) ? xb[k] : 0.f;
            }
        }
    }
    __device__ __forceinline__ void stash(int, GramLds& sm) const {
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            sm[0][sk + j][srow] = (double)ra[j];
            if (!same) sm[1][sk + j][srow] = (double)rb[j];
        }
    }
};

// thread -> column tid & 63 of both panels (columns ca0 + .. and cb0 + .. of x), rows (tid >> 6) + 4 r of the chunk; the column's
// mean is subtracted in fp64 at the stash.  Rows past N and columns past D enter as zeros.
struct ColPanels {
    typedef long long index_t;
    const float *xa, *xb;
    bool va, vb, same;
    double ma, mb;
    long long extent;
    int D, scol, srow;
    float ra[KPT], rb[KPT];
    __device__ __forceinline__ ColPanels(const float* x, const double* mean, long long N, int D_, int ca0, int cb0, bool same_)
        : same(same_), extent(N), D(D_), scol(threadIdx.x & 63), srow(threadIdx.x >> 6) {
        const int ca = ca0 + scol, cb = cb0 + scol;
        va = ca < D; vb = !same && cb < D;
        ma = va ? mean[ca] : 0.0; mb = vb ? mean[cb] : 0.0;
        xa = x + (va ? ca : 0); xb = x + (vb ? cb : 0);
    }
    __device__ __forceinline__ void fetch(long long n0) {
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const long long n = n0 + srow + 4 * r;
            const bool in = n < extent;
            ra[r] = (va && in) ? xa[(size_t)n * D] : 0.f;
            rb[r] = (vb && in) ? xb[(size_t)n * D] : 0.f;
        }
    }
    __device__ __forceinline__ void stash(long long n0, GramLds& sm) const {
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const bool in = n0 + srow + 4 * r < extent;
            sm[0][srow + 4 * r][scol] = (va && in) ? (double)ra[r] - ma : 0.0;
        }
        if (same) return;
#pragma unroll
        for (int r = 0; r < KPT; ++r) {
            const bool in = n0 + srow + 4 * r < extent;
            sm[1][srow + 4 * r][scol] = (vb && in) ? (double)rb[r] - mb : 0.0;
        }
    }
};

// The tile loop.  src by value: its staging registers live in the loop and nowhere else.  Ends behind a barrier: sm is free on
// return.
template <class Panels>
__device__ __forceinline__ void gram64_tile(Panels src, GramLds& sm, f64x4 (&acc)[2][2]) {
    typedef typename Panels::index_t index_t;
    const GramLane q;
    const double* qa = &sm[0][q.lk][q.wr * 32 + q.lc];
    const double* qb = &sm[src.same ? 0 : 1][q.lk][q.wc * 32 + q.lc];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};

    src.fetch(0);
    for (index_t k0 = 0; k0 < src.extent; k0 += KC) {
        src.stash(k0, sm);
        __syncthreads();
        if (k0 + KC < src.extent) src.fetch(k0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a0 = qa[kk * 4 * LDW], a1 = qa[kk * 4 * LDW + 16];
            const double b0 = qb[kk * 4 * LDW], b1 = qb[kk * 4 * LDW + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
}
#endif
