// mogan_knn.hip -- what improved precision / recall and density / coverage of DESIGN.md section 9f are computed from: k-nearest-
// neighbour radii inside a set of codes and ball membership between two sets, on squared Euclidean distances
//
//   d2(a, b) = max((|a|^2 + |b|^2) - 2 <a, b>, 0)
//
// of fp32 rows, widened exactly; everything after the load is fp64 and no distance matrix is ever written.  The reference
// repository has no code for this.
//
// gram_tile: one 64 x 64 tile of <a_i, b_j> per 4-wave block, gram64_tile of csrc/mogan_gram64.h on two row panels, for the three
// kernels below; the K steps run along the feature axis in index order; rows past the set and features past D enter as zeros.
//
// The scores are decisions (<=), so two properties are part of the contract:
//   * a distance's bits depend on the two rows only -- not on the tile, the wave, or which operand a row is.  The products of an
//     MFMA commute and every accumulator sees the same K steps in the same order, so <a, b> has that property; the row norms are
//     the DIAGONAL of the same tile loop run on a 64-row group against itself (row_norm_kernel, one launch per set into the
//     workspace), never a scalar fma chain.  A bit copy of a row is then at (n + n) - 2 n = 0 exactly, d2(i, j) = d2(j, i) bitwise
//     and a permutation of the rows permutes the results bitwise.
//   * no atomics; the same inputs give the same bits on every call.
//
// knn_kernel: a block owns a 64-row stripe and walks the column tiles of its share (grid.y shares where the stripes alone would
// not fill the device).  Per tile the distances go through LDS (the staging image, free after the loop) to one thread per row,
// which keeps the 8 smallest in registers, sorted (compare against the 8th, insert); j = i by POSITION and columns past N are
// left out.  The K smallest of a share go to the workspace and knn_merge_kernel merges the shares per row: the K smallest values
// of a multiset do not depend on how it was partitioned.
//
// ball_kernel: a block owns a 64-query stripe and walks the support tiles of its share; a lane counts d2 <= r2 for its 8 rows x
// R radii in registers over all its tiles, the 16 lanes of a row meet by a fixed butterfly, the two waves of a row in LDS, the
// shares in ball_finish_kernel in share order (integers: any fixed order gives the same result).
//
// cross_kernel: knn_kernel between two sets and with the positions -- a block owns a 64-query stripe and
// walks the support tiles of its share; the selecting thread keeps the 8 first (d2, i) pairs in registers under the lexicographic
// order `before` (by distance, equal bits by position), which is a total order on the pairs of a row: the K first of a set of
// pairs do not depend on how it was partitioned, so cross_merge_kernel merges the shares' lists under the same order.
//
// LABEL (mogan_knn_label_f64): the same two kernels with an int32 label per query and per bank row.  Beside
// the K list, which the labels play no part in, a selecting thread keeps the first pair under `before` among the rows of its
// query's label and the first among all other rows -- two more (d2, i) pairs in registers, the tile's 64 bank labels in LDS.  The
// first of a set under a total order does not depend on the partition either, so the shares' pairs merge like the lists.  An
// empty set keeps (+inf, NO_ROW).  The score's rows are short (D = 256, 768), so selection counts: in the LABEL instantiations
// all four waves select, a quarter of a tile's columns each for the 64 queries, keep their lists over the share's tiles and meet
// in LDS behind the loop, where wave 0 merges them under the same order (measured: DESIGN.md section 9m).  Without LABEL one wave
// selects: mogan_knn_cross_f64's path, whose timing that section holds to its parent's.
#include <hip/hip_runtime.h>
#include <cmath>
#include "mogan_gram64.h"

namespace {

constexpr int LDD = CT + 1;    // row stride of the distance tile in LDS
constexpr int K_MAX = 8;
constexpr int R_MAX = 4;
constexpr int SPLIT_BLOCKS = 512;   // shares are added until the grid has this many blocks
constexpr int SPLIT_MAX = 64;

static_assert(CT * LDD <= 2 * KC * LDW, "the distance tile lives in the staging image");

__host__ __device__ static inline long long tiles_of(long long n) { return (n + CT - 1) / CT; }

// the number of shares the column tiles are split into: a function of the two tile counts only
static inline int shares_of(long long rows, long long cols) {
    const long long tr = tiles_of(rows), tc = tiles_of(cols);
    long long s = (SPLIT_BLOCKS + tr - 1) / tr;
    if (s > tc) s = tc;
    if (s > SPLIT_MAX) s = SPLIT_MAX;
    return s < 1 ? 1 : (int)s;
}

// acc = <a_i, b_j> for rows a0 .. a0 + 63 of A against rows b0 .. b0 + 63 of B.  `same`: B's panel is A's (one panel staged).
// Ends behind a barrier: sm is free on return.
template <bool VEC>
__device__ __forceinline__ void gram_tile(const float* __restrict__ A, long long NA, long long a0, const float* __restrict__ B,
                                          long long NB, long long b0, int D, bool same, GramLds& sm, f64x4 (&acc)[2][2]) {
    const long long pa = a0 + RowPanels<VEC>::stage_row(), pb = b0 + RowPanels<VEC>::stage_row();
    const bool va = pa < NA, vb = !same && pb < NB;
    RowPanels<VEC> src(A + (size_t)(va ? pa : 0) * D, va, B + (size_t)(vb ? pb : 0) * D, vb, D, same);
    gram64_tile(src, sm, acc);
}

// the one expression of a distance: symmetric in (na, nb), exactly 0 where na == nb == g
__device__ __forceinline__ double sqdist(double na, double nb, double g) {
#pragma clang fp contract(off)
    const double s = na + nb;
    const double t = 2.0 * g;
    return fmax(s - t, 0.0);
}

// norms[i] = <x_i, x_i> as the diagonal of gram_tile on rows 64 b .. 64 b + 63 against themselves
template <bool VEC>
__global__ __launch_bounds__(NT) void row_norm_kernel(const float* __restrict__ x, long long N, int D,
                                                      double* __restrict__ norms) {
    __shared__ GramLds sm;
    const long long r0 = (long long)blockIdx.x * CT;
    f64x4 acc[2][2];
    gram_tile<VEC>(x, N, r0, x, N, r0, D, true, sm, acc);
    const GramLane ln;
    if (ln.wr != ln.wc) return;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ln.lk + 4 * j == ln.lc) {                              // row == column inside the 16 x 16 tile (m, m)
                const long long row = ln.col(r0, m);                   // of a diagonal quarter: its row as well
                if (row < N) norms[row] = acc[m][m][j];
            }
}

// v into the sorted list of the 8 smallest (the caller has seen v < best[7])
__device__ __forceinline__ void insert8(double (&best)[K_MAX], double v) {
    best[K_MAX - 1] = v;
#pragma unroll
    for (int t = K_MAX - 1; t > 0; --t) {
        const double lo = fmin(best[t - 1], best[t]), hi = fmax(best[t - 1], best[t]);
        best[t - 1] = lo;
        best[t] = hi;
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void knn_kernel(const float* __restrict__ x, long long N, int D, int K,
                                                 const double* __restrict__ norms, double* __restrict__ part) {
    __shared__ GramLds sm;
    const int tid = threadIdx.x;
    const GramLane ln;
    const long long r0 = (long long)blockIdx.x * CT;
    const long long T = tiles_of(N);
    const long long t_lo = T * blockIdx.y / gridDim.y, t_hi = T * (blockIdx.y + 1) / gridDim.y;
    double na[8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long row = ln.row(r0, m, j);
            na[m * 4 + j] = row < N ? norms[row] : 0.0;
        }
    double best[K_MAX];
#pragma unroll
    for (int t = 0; t < K_MAX; ++t) best[t] = INFINITY;
    double* dist = &sm[0][0][0];
    const long long own = r0 + tid;                                    // the row of the selecting thread (tid < 64)
    f64x4 acc[2][2];
    for (long long bt = t_lo; bt < t_hi; ++bt) {
        const long long c0 = bt * CT;
        gram_tile<VEC>(x, N, r0, x, N, c0, D, false, sm, acc);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int cl = ln.col(0, n);
            const double nb = c0 + cl < N ? norms[c0 + cl] : 0.0;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) dist[ln.row(0, m, j) * LDD + cl] = sqdist(na[m * 4 + j], nb, acc[m][n][j]);
        }
        __syncthreads();
        if (tid < CT) {
            const long long lim = N - c0 < CT ? N - c0 : CT;
            for (int c = 0; c < (int)lim; ++c) {
                const double v = dist[tid * LDD + c];
                if (c0 + c != own && v < best[K_MAX - 1]) insert8(best, v);
            }
        }
        __syncthreads();
    }
    if (tid < CT && own < N) {
        double* o = part + ((size_t)blockIdx.y * (size_t)N + (size_t)own) * K;
#pragma unroll
        for (int t = 0; t < K_MAX; ++t)
            if (t < K) o[t] = best[t];
    }
}

__global__ __launch_bounds__(NT) void knn_merge_kernel(const double* __restrict__ part, long long N, int K, int shares,
                                                       double* __restrict__ out) {
    const long long row = (long long)blockIdx.x * NT + threadIdx.x;
    if (row >= N) return;
    double best[K_MAX];
#pragma unroll
    for (int t = 0; t < K_MAX; ++t) best[t] = INFINITY;
    for (int s = 0; s < shares; ++s) {
        const double* p = part + ((size_t)s * (size_t)N + (size_t)row) * K;
        for (int t = 0; t < K; ++t) {
            const double v = p[t];
            if (v < best[K_MAX - 1]) insert8(best, v);
        }
    }
    double* o = out + (size_t)row * K;
#pragma unroll
    for (int t = 0; t < K_MAX; ++t)
        if (t < K) o[t] = best[t];
}

// (v, i) comes before (w, j) in a neighbour list: by distance, equal bits by position
__device__ __forceinline__ bool before(double v, int32_t i, double w, int32_t j) { return v < w || (v == w && i < j); }

// (v, i) into the list of the 8 first pairs under `before` (the caller has seen it before the 8th)
__device__ __forceinline__ void insert8(double (&best)[K_MAX], int32_t (&at)[K_MAX], double v, int32_t i) {
    best[K_MAX - 1] = v;
    at[K_MAX - 1] = i;
#pragma unroll
    for (int t = K_MAX - 1; t > 0; --t) {
        const bool up = before(best[t], at[t], best[t - 1], at[t - 1]);
        const double lo = up ? best[t] : best[t - 1], hi = up ? best[t - 1] : best[t];
        const int32_t li = up ? at[t] : at[t - 1], hi_i = up ? at[t - 1] : at[t];
        best[t - 1] = lo; best[t] = hi;
        at[t - 1] = li; at[t] = hi_i;
    }
}

// an empty slot: after every pair a set can hold (positions end at 2^31 - 2), so a share of fewer than K columns merges as it is
constexpr int32_t NO_ROW = 2147483647;

// LABEL: lab_d / lab_at (shares, M, 2) hold a share's first pair among the rows of the query's label [0] and among the others [1]
template <bool VEC, bool LABEL>
__global__ __launch_bounds__(NT) void cross_kernel(const float* __restrict__ q, long long M, const float* __restrict__ p, long long N,
                                                   int D, int K, const double* __restrict__ nq, const double* __restrict__ np,
                                                   double* __restrict__ part, int32_t* __restrict__ part_at,
                                                   const int32_t* __restrict__ qlabel, const int32_t* __restrict__ plabel,
                                                   double* __restrict__ lab_d, int32_t* __restrict__ lab_at) {
    __shared__ GramLds sm;
    int32_t* lab = nullptr;                                            // the tile's bank labels
    if constexpr (LABEL) {
        __shared__ int32_t lab_s[CT];
        lab = lab_s;
    }
    const int tid = threadIdx.x;
    const GramLane ln;
    const long long r0 = (long long)blockIdx.x * CT;
    const long long T = tiles_of(N);
    const long long t_lo = T * blockIdx.y / gridDim.y, t_hi = T * (blockIdx.y + 1) / gridDim.y;
    double na[8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long row = ln.row(r0, m, j);
            na[m * 4 + j] = row < M ? nq[row] : 0.0;
        }
    double best[K_MAX];
    int32_t at[K_MAX];
#pragma unroll
    for (int t = 0; t < K_MAX; ++t) {
        best[t] = INFINITY;
        at[t] = NO_ROW;
    }
    double* dist = &sm[0][0][0];
    // SEL waves select: wave w takes the tile's columns [w CT / SEL, (w + 1) CT / SEL) for the 64 queries, one query per lane
    constexpr int SEL = LABEL ? NT / CT : 1, COLS = CT / SEL;
    const int srow = SEL > 1 ? tid & (CT - 1) : tid, sw = SEL > 1 ? tid / CT : 0;      // one wave: the row is the thread
    const bool selects = tid < CT * SEL;
    const long long own = r0 + srow;                                   // the query of a selecting thread
    double ld[2] = {INFINITY, INFINITY};                               // [0] the query's label, [1] any other
    int32_t la[2] = {NO_ROW, NO_ROW};
    int32_t ql = 0;
    if constexpr (LABEL) ql = own < M ? qlabel[own] : 0;
    f64x4 acc[2][2];
    for (long long bt = t_lo; bt < t_hi; ++bt) {
        const long long c0 = bt * CT;
        gram_tile<VEC>(q, M, r0, p, N, c0, D, false, sm, acc);
        if constexpr (LABEL)
            if (tid < CT) lab[tid] = c0 + tid < N ? plabel[c0 + tid] : 0;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int cl = ln.col(0, n);
            const double nb = c0 + cl < N ? np[c0 + cl] : 0.0;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) dist[ln.row(0, m, j) * LDD + cl] = sqdist(na[m * 4 + j], nb, acc[m][n][j]);
        }
        __syncthreads();
        if (selects) {
            const long long lim = N - c0 < CT ? N - c0 : CT;
            const int c_hi = SEL > 1 && (sw + 1) * COLS < (int)lim ? (sw + 1) * COLS : (int)lim;
            for (int c = sw * COLS; c < c_hi; ++c) {
                const double v = dist[srow * LDD + c];
                const int32_t i = (int32_t)(c0 + c);
                if (before(v, i, best[K_MAX - 1], at[K_MAX - 1])) insert8(best, at, v, i);
                if constexpr (LABEL) {
                    const bool mine = lab[c] == ql;
                    const bool first = before(v, i, mine ? ld[0] : ld[1], mine ? la[0] : la[1]);
                    if (first && mine) { ld[0] = v; la[0] = i; }
                    if (first && !mine) { ld[1] = v; la[1] = i; }
                }
            }
        }
        __syncthreads();
    }
    if constexpr (SEL > 1) {
        // the waves' lists of a query meet in LDS (the distance tile is free behind the loop's last barrier) and wave 0 merges them
        // under the same order: [wave - 1][slot][query], the K lists' K_MAX slots first, then the two label pairs
        constexpr int SLOTS = K_MAX + 2;
        static_assert((SEL - 1) * SLOTS * CT * 3 <= 2 * 2 * KC * LDW, "the waves' lists live in the staging image");
        double* md = dist;
        int32_t* mi = (int32_t*)(dist + (SEL - 1) * SLOTS * CT);
        if (sw > 0) {
            const int o = (sw - 1) * SLOTS * CT + srow;
#pragma unroll
            for (int t = 0; t < K_MAX; ++t) {
                md[o + t * CT] = best[t];
                mi[o + t * CT] = at[t];
            }
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                md[o + (K_MAX + w) * CT] = ld[w];
                mi[o + (K_MAX + w) * CT] = la[w];
            }
        }
        __syncthreads();
        if (sw == 0) {
            for (int s = 0; s < SEL - 1; ++s) {
                const int o = s * SLOTS * CT + srow;
#pragma unroll
                for (int t = 0; t < K_MAX; ++t) {
                    const double v = md[o + t * CT];
                    const int32_t i = mi[o + t * CT];
                    if (before(v, i, best[K_MAX - 1], at[K_MAX - 1])) insert8(best, at, v, i);
                }
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const double v = md[o + (K_MAX + w) * CT];
                    const int32_t i = mi[o + (K_MAX + w) * CT];
                    if (before(v, i, ld[w], la[w])) { ld[w] = v; la[w] = i; }
                }
            }
        }
    }
    if (tid < CT && own < M) {
        const size_t o = ((size_t)blockIdx.y * (size_t)M + (size_t)own) * K;
#pragma unroll
        for (int t = 0; t < K_MAX; ++t)
            if (t < K) {
                part[o + t] = best[t];
                part_at[o + t] = at[t];
            }
        if constexpr (LABEL) {
            const size_t l = ((size_t)blockIdx.y * (size_t)M + (size_t)own) * 2;
            lab_d[l] = ld[0]; lab_d[l + 1] = ld[1];
            lab_at[l] = la[0]; lab_at[l + 1] = la[1];
        }
    }
}

template <bool LABEL>
__global__ __launch_bounds__(NT) void cross_merge_kernel(const double* __restrict__ part, const int32_t* __restrict__ part_at,
                                                         long long M, int K, int shares, double* __restrict__ d2,
                                                         int32_t* __restrict__ idx, const double* __restrict__ lab_d,
                                                         const int32_t* __restrict__ lab_at, double* __restrict__ same_d2,
                                                         int32_t* __restrict__ same_idx, double* __restrict__ other_d2,
                                                         int32_t* __restrict__ other_idx) {
    const long long row = (long long)blockIdx.x * NT + threadIdx.x;
    if (row >= M) return;
    double best[K_MAX];
    int32_t at[K_MAX];
#pragma unroll
    for (int t = 0; t < K_MAX; ++t) {
        best[t] = INFINITY;
        at[t] = NO_ROW;
    }
    for (int s = 0; s < shares; ++s) {
        const size_t o = ((size_t)s * (size_t)M + (size_t)row) * K;
        for (int t = 0; t < K; ++t) {
            const double v = part[o + t];
            const int32_t i = part_at[o + t];
            if (before(v, i, best[K_MAX - 1], at[K_MAX - 1])) insert8(best, at, v, i);
        }
    }
    const size_t o = (size_t)row * K;
#pragma unroll
    for (int t = 0; t < K_MAX; ++t)
        if (t < K) {
            d2[o + t] = best[t];
            idx[o + t] = at[t];
        }
    if constexpr (LABEL) {
        double ld[2] = {INFINITY, INFINITY};
        int32_t la[2] = {NO_ROW, NO_ROW};
        for (int s = 0; s < shares; ++s) {
            const size_t l = ((size_t)s * (size_t)M + (size_t)row) * 2;
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const double v = lab_d[l + w];
                const int32_t i = lab_at[l + w];
                if (before(v, i, ld[w], la[w])) { ld[w] = v; la[w] = i; }
            }
        }
        same_d2[row] = ld[0]; same_idx[row] = la[0];
        other_d2[row] = ld[1]; other_idx[row] = la[1];
    }
}

// SIDE 0: the radius belongs to the support point (r2 (N, R), by column); SIDE 1: to the query (r2 (M, R), by row)
template <bool VEC, int SIDE>
__global__ __launch_bounds__(NT) void ball_kernel(const float* __restrict__ q, long long M, const float* __restrict__ p, long long N,
                                                  int D, const double* __restrict__ r2, int R, const double* __restrict__ nq,
                                                  const double* __restrict__ np, int32_t* __restrict__ part) {
    __shared__ GramLds sm;
    __shared__ double rq[CT][R_MAX];
    __shared__ int32_t red[2][CT][R_MAX];
    const int tid = threadIdx.x;
    const GramLane ln;
    const long long r0 = (long long)blockIdx.x * CT;
    const long long T = tiles_of(N);
    const long long t_lo = T * blockIdx.y / gridDim.y, t_hi = T * (blockIdx.y + 1) / gridDim.y;
    // a radius of -1 counts nothing (d2 >= 0): radii past R, past M, past N
    if (SIDE == 1) {
        const int rl = tid >> 2, c = tid & 3;
        rq[rl][c] = (c < R && r0 + rl < M) ? r2[(size_t)(r0 + rl) * R + c] : -1.0;
    }
    double na[8];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long row = ln.row(r0, m, j);
            na[m * 4 + j] = row < M ? nq[row] : 0.0;
        }
    int32_t cnt[8][R_MAX];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < R_MAX; ++c) cnt[i][c] = 0;
    f64x4 acc[2][2];
    for (long long bt = t_lo; bt < t_hi; ++bt) {
        const long long c0 = bt * CT;
        gram_tile<VEC>(q, M, r0, p, N, c0, D, false, sm, acc);         // its barriers also order rq's fill before its use
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const long long col = ln.col(c0, n);
            const bool vc = col < N;
            const double nb = vc ? np[col] : 0.0;
            double rr[R_MAX];
#pragma unroll
            for (int c = 0; c < R_MAX; ++c) rr[c] = (SIDE == 0 && vc && c < R) ? r2[(size_t)col * R + c] : -1.0;
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int rl = ln.row(0, m, j);
                    const double d = sqdist(na[m * 4 + j], nb, acc[m][n][j]);
#pragma unroll
                    for (int c = 0; c < R_MAX; ++c) {
                        const double r = SIDE == 1 ? rq[rl][c] : rr[c];
                        cnt[m * 4 + j][c] += (vc && d <= r) ? 1 : 0;
                    }
                }
        }
    }
    // the 16 lanes of a row (same lane >> 4), then the two waves of a row
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < R_MAX; ++c) {
            int32_t v = cnt[i][c];
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
            cnt[i][c] = v;
        }
    if (ln.lc == 0) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < R_MAX; ++c) red[ln.wc][ln.row(0, m, j)][c] = cnt[m * 4 + j][c];
    }
    __syncthreads();
    {
        const int rl = tid >> 2, c = tid & 3;
        if (c < R && r0 + rl < M)
            part[((size_t)blockIdx.y * (size_t)M + (size_t)(r0 + rl)) * R + c] = red[0][rl][c] + red[1][rl][c];
    }
}

__global__ __launch_bounds__(NT) void ball_finish_kernel(const int32_t* __restrict__ part, long long MR, int shares,
                                                         int32_t* __restrict__ count) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= MR) return;
    int32_t t = 0;
    for (int s = 0; s < shares; ++s) t += part[(size_t)s * (size_t)MR + (size_t)i];
    count[i] = t;
}

static int launch_norms(const float* x, long long N, int D, double* norms, bool vec, hipStream_t stream) {
    const dim3 grid((unsigned)tiles_of(N));
    if (vec)
        hipLaunchKernelGGL(row_norm_kernel<true>, grid, dim3(NT), 0, stream, x, N, D, norms);
    else
        hipLaunchKernelGGL(row_norm_kernel<false>, grid, dim3(NT), 0, stream, x, N, D, norms);
    return ok_launch();
}

static inline size_t up8(size_t b) { return (b + 7) & ~(size_t)7; }

// the launches of mogan_knn_cross_f64 and, with LABEL, of mogan_knn_label_f64, whose workspace is the former's followed by the
// shares' label pairs: lab_d (shares, M, 2) fp64, lab_at (shares, M, 2) int32
template <bool LABEL>
static int launch_cross(const float* q, const int32_t* qlabel, long long M, const float* p, const int32_t* plabel, long long N, int D,
                        int K, double* d2, int32_t* idx, double* same_d2, int32_t* same_idx, double* other_d2, int32_t* other_idx,
                        void* ws, hipStream_t stream) {
    const bool vec = D % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)p & 15) == 0;
    const int shares = shares_of(M, N);
    const size_t lists = (size_t)shares * (size_t)M * (size_t)K;
    double* nq = (double*)ws;
    double* np = nq + M;
    double* part = np + N;
    int32_t* part_at = (int32_t*)(part + lists);
    double* lab_d = LABEL ? (double*)((char*)part_at + up8(lists * sizeof(int32_t))) : nullptr;
    int32_t* lab_at = LABEL ? (int32_t*)(lab_d + (size_t)shares * (size_t)M * 2) : nullptr;
    if (launch_norms(q, M, D, nq, vec, stream) != 0) return MOGAN_ERR_LAUNCH;
    if (launch_norms(p, N, D, np, vec, stream) != 0) return MOGAN_ERR_LAUNCH;
    const dim3 grid((unsigned)tiles_of(M), shares);
    if (vec)
        hipLaunchKernelGGL((cross_kernel<true, LABEL>), grid, dim3(NT), 0, stream, q, M, p, N, D, K, (const double*)nq,
                           (const double*)np, part, part_at, qlabel, plabel, lab_d, lab_at);
    else
        hipLaunchKernelGGL((cross_kernel<false, LABEL>), grid, dim3(NT), 0, stream, q, M, p, N, D, K, (const double*)nq,
                           (const double*)np, part, part_at, qlabel, plabel, lab_d, lab_at);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(cross_merge_kernel<LABEL>, dim3((unsigned)((M + NT - 1) / NT)), dim3(NT), 0, stream, (const double*)part,
                       (const int32_t*)part_at, M, K, shares, d2, idx, (const double*)lab_d, (const int32_t*)lab_at, same_d2,
                       same_idx, other_d2, other_idx);
    return ok_launch();
}

}  // namespace

extern "C" {

size_t mogan_knn_sqdist_ws_bytes(long long N, int K) {
    if (K < 1 || K > K_MAX || N < (long long)K + 1 || N > N_MAX) return 0;
    return ((size_t)N + (size_t)shares_of(N, N) * (size_t)N * (size_t)K) * sizeof(double);
}

int mogan_knn_sqdist_f64(const float* x, long long N, int D, int K, double* out, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!x || !out || K < 1 || K > K_MAX || N < (long long)K + 1 || N > N_MAX || D < 1 || D > D_MAX) return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_knn_sqdist_ws_bytes(N, K)) return MOGAN_ERR_WS;
    const bool vec = D % 4 == 0 && ((uintptr_t)x & 15) == 0;
    double* norms = (double*)ws;
    double* part = norms + N;
    const int shares = shares_of(N, N);
    if (launch_norms(x, N, D, norms, vec, stream) != 0) return MOGAN_ERR_LAUNCH;
    const dim3 grid((unsigned)tiles_of(N), shares);
    if (vec)
        hipLaunchKernelGGL(knn_kernel<true>, grid, dim3(NT), 0, stream, x, N, D, K, (const double*)norms, part);
    else
        hipLaunchKernelGGL(knn_kernel<false>, grid, dim3(NT), 0, stream, x, N, D, K, (const double*)norms, part);
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, (const double*)part, N, K,
                       shares, out);
    return ok_launch();
}

size_t mogan_ball_count_ws_bytes(long long M, long long N, int R) {
    if (R < 1 || R > R_MAX || M < 1 || N < 1 || M > N_MAX || N > N_MAX) return 0;
    return ((size_t)M + (size_t)N) * sizeof(double) + up8((size_t)shares_of(M, N) * (size_t)M * (size_t)R * sizeof(int32_t));
}

int mogan_ball_count_f64(const float* q, long long M, const float* p, long long N, int D, const double* r2, int R, int side,
                         int32_t* count, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!q || !p || !r2 || !count || M < 1 || N < 1 || M > N_MAX || N > N_MAX || D < 1 || D > D_MAX || R < 1 || R > R_MAX ||
        (side != 0 && side != 1))
        return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_ball_count_ws_bytes(M, N, R)) return MOGAN_ERR_WS;
    const bool vec = D % 4 == 0 && ((uintptr_t)q & 15) == 0 && ((uintptr_t)p & 15) == 0;
    double* nq = (double*)ws;
    double* np = nq + M;
    int32_t* part = (int32_t*)(np + N);
    const int shares = shares_of(M, N);
    if (launch_norms(q, M, D, nq, vec, stream) != 0) return MOGAN_ERR_LAUNCH;
    if (launch_norms(p, N, D, np, vec, stream) != 0) return MOGAN_ERR_LAUNCH;
    const dim3 grid((unsigned)tiles_of(M), shares);
#define MOGAN_BALL(V, S)                                                                                                  \
    hipLaunchKernelGGL((ball_kernel<V, S>), grid, dim3(NT), 0, stream, q, M, p, N, D, r2, R, (const double*)nq, (const double*)np, \
                       part)
    if (vec) {
        if (side == 0) MOGAN_BALL(true, 0); else MOGAN_BALL(true, 1);
    } else {
        if (side == 0) MOGAN_BALL(false, 0); else MOGAN_BALL(false, 1);
    }
#undef MOGAN_BALL
    if (ok_launch() != 0) return MOGAN_ERR_LAUNCH;
    const long long MR = M * R;
    hipLaunchKernelGGL(ball_finish_kernel, dim3((unsigned)((MR + NT - 1) / NT)), dim3(NT), 0, stream, (const int32_t*)part, MR,
                       shares, count);
    return ok_launch();
}

size_t mogan_knn_cross_ws_bytes(long long M, long long N, int K) {
    if (K < 1 || K > K_MAX || M < 1 || N < (long long)K || M > N_MAX || N > N_MAX) return 0;
    const size_t lists = (size_t)shares_of(M, N) * (size_t)M * (size_t)K;
    return ((size_t)M + (size_t)N + lists) * sizeof(double) + up8(lists * sizeof(int32_t));
}

int mogan_knn_cross_f64(const float* q, long long M, const float* p, long long N, int D, int K, double* d2, int32_t* idx, void* ws,
                        size_t ws_bytes, hipStream_t stream) {
    if (!q || !p || !d2 || !idx || K < 1 || K > K_MAX || M < 1 || N < (long long)K || M > N_MAX || N > N_MAX || D < 1 || D > D_MAX)
        return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_knn_cross_ws_bytes(M, N, K)) return MOGAN_ERR_WS;
    return launch_cross<false>(q, nullptr, M, p, nullptr, N, D, K, d2, idx, nullptr, nullptr, nullptr, nullptr, ws, stream);
}

size_t mogan_knn_label_ws_bytes(long long M, long long N, int K) {
    const size_t lists = mogan_knn_cross_ws_bytes(M, N, K);
    return lists == 0 ? 0 : lists + (size_t)shares_of(M, N) * (size_t)M * 2 * (sizeof(double) + sizeof(int32_t));
}

int mogan_knn_label_f64(const float* q, const int32_t* qlabel, long long M, const float* p, const int32_t* plabel, long long N, int D,
                        int K, double* d2, int32_t* idx, double* same_d2, int32_t* same_idx, double* other_d2, int32_t* other_idx,
                        void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!q || !qlabel || !p || !plabel || !d2 || !idx || !same_d2 || !same_idx || !other_d2 || !other_idx || K < 1 || K > K_MAX ||
        M < 1 || N < (long long)K || M > N_MAX || N > N_MAX || D < 1 || D > D_MAX)
        return MOGAN_ERR_SHAPE;
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < mogan_knn_label_ws_bytes(M, N, K)) return MOGAN_ERR_WS;
    return launch_cross<true>(q, qlabel, M, p, plabel, N, D, K, d2, idx, same_d2, same_idx, other_d2, other_idx, ws, stream);
}

}  // extern "C"
