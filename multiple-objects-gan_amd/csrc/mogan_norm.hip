// mogan_norm.hip -- BatchNorm (training statistics) fused with GLU / LeakyReLU / ReLU / residual-add,
// forward and backward, plus the eval-mode per-channel affine used by the frozen Inception trunk.
//
// All of it is HBM-bound.  Layout x (B,C,HW), NCHW.  What is computed per channel and per element -- statistics, running
// update, act(x*sc+sh), the activation backward, dx, dgamma / dbeta -- is mogan_bn.h; the kernels here only differ in how
// they spread that over blocks and launches.  Sums are fp64 (E[x^2]-mean^2 is then safe), wave64 shuffle reductions, fixed
// order; the backward recomputes the activation from x (the forward saves nothing but x, mean, invstd).  Three paths per
// direction, chosen from the shape alone:
//   one launch     bn_small_ok: B*HW <= SMALL_NE values per channel and HW >= 16.  A block per output channel (GLU: per
//                  pair) holds the channel's values in registers, reduces them and applies (bn_small_fwd / bn_small_bwd).
//                  The grouped entry points are this path with G > 1: G calls, each with its own statistics, in one launch.
//   two launches   bn_fused_ok: larger maps with HW % 4 == 0 and HW >= 64.  bn_partial / bn_bwd_partial, grid (C, YS),
//                  leave one fp64 partial sum per (batch-range x HW-range) slab; the apply kernels (bn_fwd_apply_fused /
//                  bn_bwd_apply_fused) sum a channel's partials per wave and one block per channel also writes mean /
//                  invstd / running statistics, or dgamma / dbeta.
//   three launches everything else (odd plane sizes beyond the one-launch limit, HW < 16, BatchNorm1d with its own
//                  thread-per-channel bn1d_partial): partial, bn_finalize / bn_bwd_finalize (a thread per channel), then
//                  bn_act_fwd / bn_bwd_apply.  mogan_bn_stats and mogan_bn_act_fwd are this path's two halves.
// Apply grids carry (image, channel) in gridDim.y: batches with B*Cy > 65535 go out in chunks (for_batch_chunks).
// Replaces nn.BatchNorm1d/2d + GLU / nn.LeakyReLU / nn.ReLU at code/coco/attngan/model.py:48-81,
// 96-101,364-373,575-611,667-680.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/mogan_hip.h"
#include "mogan_bn.h"

namespace {

__global__ __launch_bounds__(256) void affine_relu_bwd_out_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                                  const float* __restrict__ scale, float* __restrict__ dx,
                                                                  long long n, int C, int HW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)((i / HW) % C);
    dx[i] = y[i] > 0.f ? dy[i] * scale[c] : 0.f;
}


__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// block (256 threads) reduction of NV doubles; result valid in thread 0
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* sh /* [4*NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) sh[wave * NV + i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = sh[i] + sh[NV + i] + sh[2 * NV + i] + sh[3 * NV + i];
}

struct Split { int bs, hs, bper, hper; };   // YS = bs*hs blocks per channel

static Split make_split(int B, int C, int HW) {
    Split s;
    long long want = (1536 + C - 1) / C;                     // ~6 blocks per CU overall
    if (want < 1) want = 1;
    s.bs = (int)(want < B ? want : B);
    long long rest = (want + s.bs - 1) / s.bs;
    long long hmax = (HW + 2047) / 2048; if (hmax < 1) hmax = 1;
    s.hs = (int)(rest < hmax ? rest : hmax);
    s.bper = (B + s.bs - 1) / s.bs; s.bs = (B + s.bper - 1) / s.bper;
    s.hper = (((HW + s.hs - 1) / s.hs) + 3) & ~3; s.hs = (HW + s.hper - 1) / s.hper;
    return s;
}

// W consecutive values (W == 4: one 16-byte access, the address is 16-byte aligned)
template <int W>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[4]) {
    if (W == 4) { const float4 t = *(const float4*)p; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int W>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[4]) {
    if (W == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); else *p = v[0];
}

// -------------------------------------------------------------------------------- forward stats
__global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ x, int B, int C, int HW,
                                                         Split sp, double* __restrict__ part) {
    __shared__ double sh[8];
    const int c = blockIdx.x, ys = blockIdx.y;
    const int bi = ys / sp.hs, hi = ys % sp.hs;
    const int b0 = bi * sp.bper, b1 = min(B, b0 + sp.bper);
    const int h0 = hi * sp.hper, h1 = min(HW, h0 + sp.hper);
    double acc[2] = {0.0, 0.0};
    const bool vec = ((HW & 3) == 0);
    for (int b = b0; b < b1; ++b) {
        const float* px = x + ((size_t)b * C + c) * HW;
        if (vec) {
            for (int i = h0 + threadIdx.x * 4; i < h1; i += 1024) {
                const float4 v = *(const float4*)(px + i);
                acc[0] += (double)v.x + (double)v.y + (double)v.z + (double)v.w;
                acc[1] += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
            }
        } else {
            for (int i = h0 + threadIdx.x; i < h1; i += 256) {
                const double v = px[i];
                acc[0] += v; acc[1] += v * v;
            }
        }
    }
    block_sum<2>(acc, sh);
    if (threadIdx.x == 0) {
        part[((size_t)c * gridDim.y + ys) * 2 + 0] = acc[0];
        part[((size_t)c * gridDim.y + ys) * 2 + 1] = acc[1];
    }
}

// HW == 1 (BatchNorm1d on (B,C)): one thread per channel, coalesced across channels
__global__ __launch_bounds__(256) void bn1d_partial_kernel(const float* __restrict__ x, int B, int C,
                                                           double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0, q = 0;
    for (int b = 0; b < B; ++b) { const double v = x[(size_t)b * C + c]; s += v; q += v * v; }
    part[(size_t)c * 2] = s; part[(size_t)c * 2 + 1] = q;
}

// what a BatchNorm call leaves per channel: batch statistics for the backward, running statistics updated
__device__ __forceinline__ void write_stats(int c, float mean, float invstd, double var, double n, float momentum,
                                            float* __restrict__ mo, float* __restrict__ io, float* __restrict__ rmean,
                                            float* __restrict__ rvar) {
    mo[c] = mean; io[c] = invstd;
    bn_running_update(rmean, rvar, c, mean, var, n, momentum);
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ part, int C, int YS, double n,
                                                          float eps, float momentum, float* __restrict__ mean,
                                                          float* __restrict__ invstd, float* __restrict__ rmean,
                                                          float* __restrict__ rvar) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s = 0, q = 0;
    for (int y = 0; y < YS; ++y) { s += part[((size_t)c * YS + y) * 2]; q += part[((size_t)c * YS + y) * 2 + 1]; }
    float mu, is;
    double var;
    bn_stats_of(s, q, n, eps, mu, is, var);
    write_stats(c, mu, is, var, n, momentum, mean, invstd, rmean, rvar);
}

// Deferred running-statistics update of a BatchNorm call that ran with running_mean / running_var = NULL: from the batch
// statistics it left (mean, invstd), applied later so that the running buffers see the reference's CALL ORDER although the call's
// arithmetic ran earlier (the "wrong pair" head of a discriminator update, miscc/losses.py:152-160, evaluated with the real half
// before the fake images exist).  var = 1 / invstd^2 - eps in double (invstd is a rounded float: relative error of the variance
// <= 1.2e-7 (var + eps) / var).
__global__ __launch_bounds__(256) void bn_running_update_kernel(const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                float* __restrict__ rmean, float* __restrict__ rvar, int C, double n,
                                                                float eps, float momentum) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    if (rmean) rmean[c] = bn_running_mix(rmean[c], mean[c], momentum);
    if (rvar) {
        const double is = (double)invstd[c];
        double var = 1.0 / (is * is) - (double)eps; if (var < 0) var = 0;
        rvar[c] = bn_running_mix(rvar[c], (float)bn_unbiased(var, n), momentum);
    }
}

// -------------------------------------------------------------------------------- forward apply
// W values of one (image, channel) plane at offset i: y = act(bn(x)) (+ res).  px / pg: the plane of channel c and of its GLU
// gate channel c + Cy; pr: the residual's plane or NULL
template <int ACT, int W>
__device__ __forceinline__ void bn_fwd_vec(const float* __restrict__ px, const float* __restrict__ pg,
                                           const float* __restrict__ pr, float* __restrict__ py, int i, const BnCoef& ca,
                                           const BnCoef& cg, float slope) {
    float v[4], g[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    load_vec<W>(px + i, v);
    if (ACT == MOGAN_ACT_GLU) load_vec<W>(pg + i, g);
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = bn_fwd_elem<ACT>(v[k], g[k], ca, cg, slope);
    if (pr) {
        float r[4];
        load_vec<W>(pr + i, r);
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] += r[k];
    }
    store_vec<W>(py + i, o);
}

template <int ACT, bool VEC>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                         const float* __restrict__ invstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ res, float* __restrict__ y, int C,
                                                         int HW, float slope) {
    constexpr int W = VEC ? 4 : 1;
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.y % Cy, b = blockIdx.y / Cy;
    const int i = (blockIdx.x * 256 + threadIdx.x) * W;
    if (i >= HW) return;
    BnCoef ca, cg;
    bn_coef_pair<ACT>(mean, invstd, gamma, beta, c, Cy, ca, cg);
    const float* px = x + ((size_t)b * C + c) * HW;
    bn_fwd_vec<ACT, W>(px, px + (size_t)Cy * HW, res ? res + ((size_t)b * Cy + c) * HW : nullptr,
                       y + ((size_t)b * Cy + c) * HW, i, ca, cg, slope);
}

// -------------------------------------------------------------------------------- backward
// partial sums per (channel, ys): [sum dy_a, sum dy_a*xhat_a, sum dy_g, sum dy_g*xhat_g]
template <int ACT>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int B, int C, int HW,
                                                             Split sp, float slope, double* __restrict__ part) {
    __shared__ double sh_[16];
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.x, ys = blockIdx.y;          // c in [0, Cy)
    const int bi = ys / sp.hs, hi = ys % sp.hs;
    const int b0 = bi * sp.bper, b1 = min(B, b0 + sp.bper);
    const int h0 = hi * sp.hper, h1 = min(HW, h0 + sp.hper);
    BnCoef ca, cg;
    bn_coef_pair<ACT>(mean, invstd, gamma, beta, c, Cy, ca, cg);
    double acc[4] = {0, 0, 0, 0};
    for (int b = b0; b < b1; ++b) {
        const float* pxa = x + ((size_t)b * C + c) * HW;
        const float* pxg = pxa + (size_t)Cy * HW;
        const float* pdy = dy + ((size_t)b * Cy + c) * HW;
        if ((HW & 3) == 0) {                       // (h0, h1 are multiples of 4 then: Split::hper is)
            for (int i = h0 + threadIdx.x * 4; i < h1; i += 1024) {
                float xa[4], xg[4] = {0.f, 0.f, 0.f, 0.f}, d[4];
                load_vec<4>(pxa + i, xa); load_vec<4>(pdy + i, d);
                if (ACT == MOGAN_ACT_GLU) load_vec<4>(pxg + i, xg);
#pragma unroll
                for (int k = 0; k < 4; ++k) bn_bwd_accum<ACT>(acc, xa[k], xg[k], d[k], ca, cg, slope);
            }
            continue;
        }
        for (int i = h0 + threadIdx.x; i < h1; i += 256)
            bn_bwd_accum<ACT>(acc, pxa[i], (ACT == MOGAN_ACT_GLU) ? pxg[i] : 0.f, pdy[i], ca, cg, slope);
    }
    block_sum<4>(acc, sh_);
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)c * gridDim.y + ys) * 4;
        o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2]; o[3] = acc[3];
    }
}

// -> sums[C][2] = (sum dy_bn, sum dy_bn*xhat) as float, dgamma/dbeta
template <int ACT>
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int C, int YS,
                                                              float* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, int accumulate) {
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Cy) return;
    double a[4] = {0, 0, 0, 0};
    for (int y = 0; y < YS; ++y)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] += part[((size_t)c * YS + y) * 4 + k];
    sums[c * 2] = (float)a[0]; sums[c * 2 + 1] = (float)a[1];
    bn_write_dparam(dgamma, dbeta, c, (float)a[0], (float)a[1], accumulate);
    if (ACT == MOGAN_ACT_GLU) {
        const int cg = c + Cy;
        sums[cg * 2] = (float)a[2]; sums[cg * 2 + 1] = (float)a[3];
        bn_write_dparam(dgamma, dbeta, cg, (float)a[2], (float)a[3], accumulate);
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           const float* __restrict__ sums, float* __restrict__ dx, int C,
                                                           int HW, float slope, float inv_n) {
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.y % Cy, b = blockIdx.y / Cy, cgl = c + Cy;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    BnCoef ca, cg;
    bn_coef_pair<ACT>(mean, invstd, gamma, beta, c, Cy, ca, cg);
    const size_t ia = ((size_t)b * C + c) * HW + i, ig = ia + (size_t)Cy * HW;
    const float xa = x[ia], xg = (ACT == MOGAN_ACT_GLU) ? x[ig] : 0.f;
    float s[4] = {sums[c * 2], sums[c * 2 + 1], 0.f, 0.f};
    if (ACT == MOGAN_ACT_GLU) { s[2] = sums[cgl * 2]; s[3] = sums[cgl * 2 + 1]; }
    float oa, og;
    bn_bwd_elem<ACT>(xa, xg, dy[((size_t)b * Cy + c) * HW + i], ca, cg, slope, s, inv_n, oa, og);
    dx[ia] = oa;
    if (ACT == MOGAN_ACT_GLU) dx[ig] = og;
}


// -------------------------------------------------------------------------------- finalize folded into the apply pass
// HW % 4 == 0 maps beyond the one-launch size: the per-channel reduction of the partial sums (bn_finalize_kernel /
// bn_bwd_finalize_kernel, one tiny launch each) moves into the apply kernels -- every wave sums its channel's YS partial
// entries (lanes stride the entries, xor-butterfly: all lanes hold the same fp64 totals, no LDS, no barrier) and the block
// (first tile of the first image) also writes what the finalize kernel wrote: mean / invstd / running statistics, dgamma / dbeta.
// Two launches per direction instead of three; each block covers 4096 values of one (image, channel) plane.
__device__ __forceinline__ double wave_allsum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int NV, int STRIDE>
__device__ __forceinline__ void part_sums(const double* __restrict__ part, int c, int YS, double (&a)[NV]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] = 0.0;
    for (int y = lane; y < YS; y += 64)
#pragma unroll
        for (int k = 0; k < NV; ++k) a[k] += part[((size_t)c * YS + y) * STRIDE + k];
#pragma unroll
    for (int k = 0; k < NV; ++k) a[k] = wave_allsum(a[k]);
}

constexpr int FUSED_PER = 4096;     // values of one plane per block

// channel c's statistics from its partial sums; the writer thread leaves them as bn_finalize_kernel would
__device__ __forceinline__ BnCoef fused_coef(const double* __restrict__ part, int c, int YS, double n, float eps, float momentum,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, bool wr,
                                             float* __restrict__ mean_o, float* __restrict__ invstd_o, float* __restrict__ rmean,
                                             float* __restrict__ rvar) {
    double a[2], var;
    float mu, is;
    part_sums<2, 2>(part, c, YS, a);
    bn_stats_of(a[0], a[1], n, eps, mu, is, var);
    if (wr) write_stats(c, mu, is, var, n, momentum, mean_o, invstd_o, rmean, rvar);
    return bn_coef(mu, is, gamma, beta, c);
}

template <int ACT>
__global__ __launch_bounds__(256) void bn_fwd_apply_fused_kernel(const float* __restrict__ x, const double* __restrict__ part,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ res, float* __restrict__ y,
                                                                 float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                                                 float* __restrict__ rmean, float* __restrict__ rvar, int C, int HW,
                                                                 int YS, double n, float eps, float momentum, float slope,
                                                                 int writer) {
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.y % Cy, b = blockIdx.y / Cy;
    const bool wr = writer && blockIdx.x == 0 && b == 0 && threadIdx.x == 0;
    const BnCoef ca = fused_coef(part, c, YS, n, eps, momentum, gamma, beta, wr, mean_o, invstd_o, rmean, rvar);
    BnCoef cg = {0.f, 0.f, 0.f, 0.f};
    if (ACT == MOGAN_ACT_GLU) cg = fused_coef(part, c + Cy, YS, n, eps, momentum, gamma, beta, wr, mean_o, invstd_o, rmean, rvar);
    const float* px = x + ((size_t)b * C + c) * HW;
    float* py = y + ((size_t)b * Cy + c) * HW;
    const float* pr = res ? res + ((size_t)b * Cy + c) * HW : nullptr;
    const int i0 = blockIdx.x * FUSED_PER, i1 = min(HW, i0 + FUSED_PER);
    for (int i = i0 + threadIdx.x * 4; i < i1; i += 1024)
        bn_fwd_vec<ACT, 4>(px, px + (size_t)Cy * HW, pr, py, i, ca, cg, slope);
}

template <int ACT>
__global__ __launch_bounds__(256) void bn_bwd_apply_fused_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const double* __restrict__ part, float* __restrict__ dx,
                                                                 float* __restrict__ dgamma, float* __restrict__ dbeta, int C, int HW,
                                                                 int YS, float slope, float inv_n, int accumulate, int writer) {
    constexpr int NV = (ACT == MOGAN_ACT_GLU) ? 4 : 2;
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.y % Cy, b = blockIdx.y / Cy;
    double a[NV];
    part_sums<NV, 4>(part, c, YS, a);
    float s[4] = {(float)a[0], (float)a[1], 0.f, 0.f};
    if (ACT == MOGAN_ACT_GLU) { s[2] = (float)a[NV - 2]; s[3] = (float)a[NV - 1]; }
    if (writer && blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        bn_write_dparam(dgamma, dbeta, c, s[0], s[1], accumulate);
        if (ACT == MOGAN_ACT_GLU) bn_write_dparam(dgamma, dbeta, c + Cy, s[2], s[3], accumulate);
    }
    BnCoef ca, cg;
    bn_coef_pair<ACT>(mean, invstd, gamma, beta, c, Cy, ca, cg);
    const float* pxa = x + ((size_t)b * C + c) * HW;
    const float* pxg = pxa + (size_t)Cy * HW;
    const float* pdy = dy + ((size_t)b * Cy + c) * HW;
    float* pda = dx + ((size_t)b * C + c) * HW;
    float* pdg = pda + (size_t)Cy * HW;
    const int i0 = blockIdx.x * FUSED_PER, i1 = min(HW, i0 + FUSED_PER);
    for (int i = i0 + threadIdx.x * 4; i < i1; i += 1024) {
        float xa[4], xg[4] = {0.f, 0.f, 0.f, 0.f}, d[4], oa[4], og[4];
        load_vec<4>(pxa + i, xa); load_vec<4>(pdy + i, d);
        if (ACT == MOGAN_ACT_GLU) load_vec<4>(pxg + i, xg);
#pragma unroll
        for (int k = 0; k < 4; ++k) bn_bwd_elem<ACT>(xa[k], xg[k], d[k], ca, cg, slope, s, inv_n, oa[k], og[k]);
        store_vec<4>(pda + i, oa);
        if (ACT == MOGAN_ACT_GLU) store_vec<4>(pdg + i, og);
    }
}


// -------------------------------------------------------------------------------- one-launch BatchNorm for small maps
// B*HW <= SMALL_NE values per channel (<= 16x16 maps at B = 16; BatchNorm1d): ONE block per output channel (GLU: per pair)
// does what bn_partial + bn_finalize + bn_act_fwd (and bn_bwd_partial + finalize + apply) do in three launches -- pass 1
// reduces over the channel, pass 2 applies to the values it kept.  Same arithmetic (fp64 sums, float apply).
constexpr int SMALL_NE = 4096;
constexpr int SMALL_EPT = SMALL_NE / 256;            // values per thread (and channel of a GLU pair)
constexpr unsigned SMALL_NONE = 0xFFFFFFFFu;         // offset of a slot beyond the channel's B*HW values

template <int ACT>
__global__ __launch_bounds__(256) void bn_small_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ res,
                                                           float* __restrict__ y, float* __restrict__ mean,
                                                           float* __restrict__ invstd, float* __restrict__ rmean,
                                                           float* __restrict__ rvar, int B, int C, int HW, float eps,
                                                           float momentum, float slope, int G) {
    __shared__ double sh[16];
    __shared__ float st[4];
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.x, NE = B * HW;
    constexpr int NCH = (ACT == MOGAN_ACT_GLU) ? 2 : 1;
    // G > 1: the batch holds G groups of B images, each normalised with its OWN statistics -- G BatchNorm calls in sequence (the
    // running statistics are updated group after group, as G calls would), one launch (the object pathways)
    for (int grp = 0; grp < G; ++grp, x += (size_t)B * C * HW, y += (size_t)B * Cy * HW, mean += C, invstd += C) {
    if (grp) __syncthreads();
    float v[NCH][SMALL_EPT];
    unsigned off[SMALL_EPT];
    // a thread's <= 16 values (x2 for GLU) are loaded ONCE, all loads in flight (clamped addresses, no branch), and stay in registers
    // for the apply pass (a `for (e ...)` loop with one dependent load per iteration made this kernel 13-16 us for 4096 values)
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i) {
        const int e = threadIdx.x + 256 * i;
        const bool ok = e < NE;
        const int b = e / HW, pos = e - b * HW;
        off[i] = ok ? (unsigned)((b * C + c) * HW + pos) : SMALL_NONE;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const float t = x[ok ? (size_t)off[i] + (size_t)k * Cy * HW : 0];
            v[k][i] = ok ? t : 0.f;
        }
    }
    double acc[2 * NCH];
#pragma unroll
    for (int k = 0; k < 2 * NCH; ++k) acc[k] = 0.0;
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i)
#pragma unroll
        for (int k = 0; k < NCH; ++k) { const double t = v[k][i]; acc[2 * k] += t; acc[2 * k + 1] += t * t; }
    block_sum<2 * NCH>(acc, sh);
    if (threadIdx.x == 0) {
        const double n = (double)NE;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            float mu, is;
            double var;
            bn_stats_of(acc[2 * k], acc[2 * k + 1], n, eps, mu, is, var);
            write_stats(c + k * Cy, mu, is, var, n, momentum, mean, invstd, rmean, rvar);
            st[2 * k] = mu; st[2 * k + 1] = is;
        }
    }
    __syncthreads();
    const BnCoef ca = bn_coef(st[0], st[1], gamma, beta, c);
    BnCoef cg = {0.f, 0.f, 0.f, 0.f};
    if (ACT == MOGAN_ACT_GLU) cg = bn_coef(st[2], st[3], gamma, beta, c + Cy);
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i) {
        if (off[i] == SMALL_NONE) continue;
        const int e = threadIdx.x + 256 * i;
        const int b = e / HW, pos = e - b * HW;
        const size_t iy = ((size_t)b * Cy + c) * HW + pos;
        float t = bn_fwd_elem<ACT>(v[0][i], v[NCH - 1][i], ca, cg, slope);
        if (res) t += res[iy];
        y[iy] = t;
    }
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void bn_small_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ dx, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int B, int C, int HW, float slope,
                                                           int accumulate, int G) {
    __shared__ double sh_[16];
    __shared__ float sums[4];
    const int Cy = (ACT == MOGAN_ACT_GLU) ? C / 2 : C;
    const int c = blockIdx.x, NE = B * HW;
    for (int grp = 0; grp < G; ++grp, x += (size_t)B * C * HW, dy += (size_t)B * Cy * HW, dx += (size_t)B * C * HW, mean += C,
             invstd += C, accumulate = 1) {           // (d gamma / d beta: the groups' contributions add up)
    if (grp) __syncthreads();
    BnCoef ca, cg;
    bn_coef_pair<ACT>(mean, invstd, gamma, beta, c, Cy, ca, cg);
    double acc[4] = {0, 0, 0, 0};
    // x (both halves for GLU) and dy of a thread's <= 16 elements: loaded once, all in flight, kept for the second pass
    constexpr int NCH = (ACT == MOGAN_ACT_GLU) ? 2 : 1;
    float xv[NCH][SMALL_EPT], dv[SMALL_EPT];
    unsigned off[SMALL_EPT];
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i) {
        const int e = threadIdx.x + 256 * i;
        const bool ok = e < NE;
        const int b = e / HW, pos = e - b * HW;
        off[i] = ok ? (unsigned)((b * C + c) * HW + pos) : SMALL_NONE;
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const float t = x[ok ? (size_t)off[i] + (size_t)k * Cy * HW : 0];
            xv[k][i] = ok ? t : 0.f;
        }
        const float t = dy[ok ? ((size_t)b * Cy + c) * HW + pos : 0];
        dv[i] = ok ? t : 0.f;
    }
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i) {
        if (off[i] == SMALL_NONE) continue;
        bn_bwd_accum<ACT>(acc, xv[0][i], xv[NCH - 1][i], dv[i], ca, cg, slope);
    }
    block_sum<4>(acc, sh_);
    if (threadIdx.x == 0) {
        sums[0] = (float)acc[0]; sums[1] = (float)acc[1]; sums[2] = (float)acc[2]; sums[3] = (float)acc[3];
        bn_write_dparam(dgamma, dbeta, c, sums[0], sums[1], accumulate);
        if (ACT == MOGAN_ACT_GLU) bn_write_dparam(dgamma, dbeta, c + Cy, sums[2], sums[3], accumulate);
    }
    __syncthreads();
    const float inv_n = 1.f / ((float)B * (float)HW);
    const float s[4] = {sums[0], sums[1], sums[2], sums[3]};
#pragma unroll
    for (int i = 0; i < SMALL_EPT; ++i) {
        if (off[i] == SMALL_NONE) continue;
        const size_t ia = off[i], ig = ia + (size_t)Cy * HW;
        float oa, og;
        bn_bwd_elem<ACT>(xv[0][i], xv[NCH - 1][i], dv[i], ca, cg, slope, s, inv_n, oa, og);
        dx[ia] = oa;
        if (ACT == MOGAN_ACT_GLU) dx[ig] = og;
    }
    }
}

// -------------------------------------------------------------------------------- eval affine
template <int ACT, bool BWD>
__global__ __launch_bounds__(256) void affine_act_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift, float* __restrict__ out, int C,
                                                         int HW, float slope) {
    const int c = blockIdx.y % C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const size_t idx = (size_t)blockIdx.y * HW + i;
    const BnCoef k = {0.f, 0.f, scale[c], shift[c]};
    if (!BWD) {
        out[idx] = bn_fwd_elem<ACT>(x[idx], 0.f, k, k, slope);
    } else {
        float d, dg;
        act_bwd<ACT>(x[idx], 0.f, dy[idx], k, k, slope, d, dg);
        out[idx] = d * k.sc;
    }
}

// -------------------------------------------------------------------------------- host side
static inline int ok_launch() { return hipGetLastError() == hipSuccess ? 0 : MOGAN_ERR_LAUNCH; }

// (an activation code with_act has no kernel for is refused here, before an entry point's first launch)
static bool bn_shape_ok(int B, int C, int HW, int act = MOGAN_ACT_NONE) {
    return B > 0 && C > 0 && HW > 0 && act >= MOGAN_ACT_NONE && act <= MOGAN_ACT_GLU && !(act == MOGAN_ACT_GLU && (C & 1));
}
// path selection (BatchNorm1d, HW == 1, keeps its thread-per-channel kernels: a block per channel would be 16 values wide)
static bool bn_fused_ok(int HW) { return (HW & 3) == 0 && HW >= 64; }
static bool bn_small_ok(int B, int C, int HW) { return HW >= 16 && (long long)B * HW <= SMALL_NE && C <= 65535 * 2; }

// f(std::integral_constant<int, ACT>) for the activation code `act`: the one place a kernel template meets the runtime code.
// GLU_OK = false: the kernels of the caller have no GLU form
template <bool GLU_OK = true, typename F>
static int with_act(int act, F&& f) {
    switch (act) {
        case MOGAN_ACT_NONE: return f(std::integral_constant<int, MOGAN_ACT_NONE>{});
        case MOGAN_ACT_RELU: return f(std::integral_constant<int, MOGAN_ACT_RELU>{});
        case MOGAN_ACT_LRELU: return f(std::integral_constant<int, MOGAN_ACT_LRELU>{});
        case MOGAN_ACT_GLU:
            if constexpr (GLU_OK) return f(std::integral_constant<int, MOGAN_ACT_GLU>{});
            return MOGAN_ERR_SHAPE;
        default: return MOGAN_ERR_SHAPE;
    }
}

// the apply grids carry (image, channel) in gridDim.y <= 65535: f(b0, nb) for consecutive ranges of whole images
template <typename F>
static int for_batch_chunks(int B, int Cy, F&& f) {
    const int bchunk = 65535 / Cy;
    if (bchunk < 1) return MOGAN_ERR_SHAPE;
    for (int b0 = 0; b0 < B; b0 += bchunk) f(b0, B - b0 < bchunk ? B - b0 : bchunk);
    return ok_launch();
}

// the one-launch path: G groups of B images (G == 1: one BatchNorm call)
static int launch_small_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y, float* mean,
                            float* invstd, float* running_mean, float* running_var, int B, int C, int HW, int act, float slope,
                            float eps, float momentum, int G, hipStream_t stream) {
    return with_act(act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
        hipLaunchKernelGGL((bn_small_fwd_kernel<ACT>), dim3(ACT == MOGAN_ACT_GLU ? C / 2 : C), dim3(256), 0, stream, x, gamma, beta,
                           residual, y, mean, invstd, running_mean, running_var, B, C, HW, eps, momentum, slope, G);
        return ok_launch();
    });
}
static int launch_small_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int act, float slope,
                            int accumulate, int G, hipStream_t stream) {
    return with_act(act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
        hipLaunchKernelGGL((bn_small_bwd_kernel<ACT>), dim3(ACT == MOGAN_ACT_GLU ? C / 2 : C), dim3(256), 0, stream, x, dy, mean,
                           invstd, gamma, beta, dx, dgamma, dbeta, B, C, HW, slope, accumulate, G);
        return ok_launch();
    });
}

template <bool BWD>
static int affine_impl(const float* x, const float* dy, const float* scale, const float* shift, float* out, int B,
                       int C, int HW, int act, float slope, hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW)) return MOGAN_ERR_SHAPE;
    return with_act<false>(act, [&](auto A) {
        return for_batch_chunks(B, C, [&](int b0, int nb) {
            const size_t off = (size_t)b0 * C * HW;
            hipLaunchKernelGGL((affine_act_kernel<decltype(A)::value, BWD>), dim3((HW + 255) / 256, nb * C), dim3(256), 0, stream,
                               x + off, dy ? dy + off : nullptr, scale, shift, out + off, C, HW, slope);
        });
    });
}

}  // namespace

extern "C" {

size_t mogan_bn_ws_bytes(int B, int C, int HW) {
    if (!bn_shape_ok(B, C, HW)) return 0;
    const Split s = make_split(B, C, HW);
    return (size_t)C * s.bs * s.hs * 4 * sizeof(double) + (size_t)C * 2 * sizeof(float) + 64;
}

int mogan_bn_stats(const float* x, int B, int C, int HW, float eps, float momentum, float* mean, float* invstd,
                   float* running_mean, float* running_var, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW)) return MOGAN_ERR_SHAPE;
    if (!ws || ws_bytes < mogan_bn_ws_bytes(B, C, HW)) return MOGAN_ERR_WS;
    double* part = (double*)ws;
    int YS = 1;
    if (HW == 1) {
        hipLaunchKernelGGL(bn1d_partial_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, x, B, C, part);
    } else {
        const Split s = make_split(B, C, HW);
        YS = s.bs * s.hs;
        if (YS > 65535) return MOGAN_ERR_SHAPE;
        hipLaunchKernelGGL(bn_partial_kernel, dim3(C, YS), dim3(256), 0, stream, x, B, C, HW, s, part);
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, (const double*)part, C, YS,
                       (double)B * HW, eps, momentum, mean, invstd, running_mean, running_var);
    return ok_launch();
}

int mogan_bn_running_update(const float* mean, const float* invstd, float* running_mean, float* running_var, int C, long long n,
                            float eps, float momentum, hipStream_t stream) {
    if (!mean || !invstd || C <= 0 || n <= 0) return MOGAN_ERR_SHAPE;
    hipLaunchKernelGGL(bn_running_update_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, mean, invstd, running_mean,
                       running_var, C, (double)n, eps, momentum);
    return ok_launch();
}

// statistics + apply in one call, by the path the shape selects (file head).  mean / invstd are written for the backward as by
// mogan_bn_stats.
int mogan_bn_act_fwd_fused(const float* x, const float* gamma, const float* beta, const float* residual, float* running_mean,
                           float* running_var, float* mean, float* invstd, float* y, int B, int C, int HW, int act, float slope,
                           float eps, float momentum, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW, act)) return MOGAN_ERR_SHAPE;
    const int Cy = act == MOGAN_ACT_GLU ? C / 2 : C;
    if (bn_small_ok(B, C, HW))
        return launch_small_fwd(x, gamma, beta, residual, y, mean, invstd, running_mean, running_var, B, C, HW, act, slope, eps,
                                momentum, 1, stream);
    if (Cy > 65535) return MOGAN_ERR_SHAPE;           // (no apply grid holds one image: for_batch_chunks would say so after the statistics)
    if (!bn_fused_ok(HW)) {
        int rc = mogan_bn_stats(x, B, C, HW, eps, momentum, mean, invstd, running_mean, running_var, ws, ws_bytes, stream);
        return rc ? rc : mogan_bn_act_fwd(x, mean, invstd, gamma, beta, residual, y, B, C, HW, act, slope, stream);
    }
    if (!ws || ws_bytes < mogan_bn_ws_bytes(B, C, HW)) return MOGAN_ERR_WS;
    const Split s = make_split(B, C, HW);
    const int YS = s.bs * s.hs;
    if (YS > 65535) return MOGAN_ERR_SHAPE;
    double* part = (double*)ws;
    hipLaunchKernelGGL(bn_partial_kernel, dim3(C, YS), dim3(256), 0, stream, x, B, C, HW, s, part);
    return with_act(act, [&](auto A) {
        return for_batch_chunks(B, Cy, [&](int b0, int nb) {
            hipLaunchKernelGGL((bn_fwd_apply_fused_kernel<decltype(A)::value>), dim3((HW + FUSED_PER - 1) / FUSED_PER, nb * Cy),
                               dim3(256), 0, stream, x + (size_t)b0 * C * HW, (const double*)part, gamma, beta,
                               residual ? residual + (size_t)b0 * Cy * HW : nullptr, y + (size_t)b0 * Cy * HW, mean, invstd,
                               running_mean, running_var, C, HW, YS, (double)B * HW, eps, momentum, slope, b0 == 0 ? 1 : 0);
        });
    });
}

// G BatchNorm(train) + activation calls on the G groups of B images of one (G*B, C, HW) tensor in ONE launch each way: group g is
// normalised with its own batch statistics (mean / invstd: G x C, group-major), the running statistics are updated G times in group
// order, d gamma / d beta sum over the groups.  Needs B*HW <= 4096 values per channel and group (any HW >= 1).
int mogan_bn_act_grouped_eligible(int G, int B, int C, int HW) {
    return G >= 1 && B >= 1 && C >= 1 && HW >= 1 && (long long)B * HW <= SMALL_NE && C <= 65535 * 2 &&
           (long long)G * B * C * HW < (1ll << 31) ? 1 : 0;
}

int mogan_bn_act_grouped_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* mean,
                             float* invstd, float* y, int G, int B, int C, int HW, int act, float slope, float eps, float momentum,
                             hipStream_t stream) {
    if (!mogan_bn_act_grouped_eligible(G, B, C, HW) || !bn_shape_ok(B, C, HW, act)) return MOGAN_ERR_SHAPE;
    return launch_small_fwd(x, gamma, beta, nullptr, y, mean, invstd, running_mean, running_var, B, C, HW, act, slope, eps, momentum,
                            G, stream);
}

int mogan_bn_act_grouped_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             float* dx, float* dgamma, float* dbeta, int G, int B, int C, int HW, int act, float slope, int accumulate,
                             hipStream_t stream) {
    if (!mogan_bn_act_grouped_eligible(G, B, C, HW) || !bn_shape_ok(B, C, HW, act)) return MOGAN_ERR_SHAPE;
    return launch_small_bwd(x, dy, mean, invstd, gamma, beta, dx, dgamma, dbeta, B, C, HW, act, slope, accumulate, G, stream);
}

int mogan_bn_act_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                     const float* residual, float* y, int B, int C, int HW, int act, float slope, hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW, act)) return MOGAN_ERR_SHAPE;
    const int Cy = act == MOGAN_ACT_GLU ? C / 2 : C;
    return with_act(act, [&](auto A) {
        return for_batch_chunks(B, Cy, [&](int b0, int nb) {
            constexpr int ACT = decltype(A)::value;
            const float* px = x + (size_t)b0 * C * HW;
            const float* pr = residual ? residual + (size_t)b0 * Cy * HW : nullptr;
            float* py = y + (size_t)b0 * Cy * HW;
            if ((HW & 3) == 0)
                hipLaunchKernelGGL((bn_act_fwd_kernel<ACT, true>), dim3((HW + 1023) / 1024, nb * Cy), dim3(256), 0, stream, px, mean,
                                   invstd, gamma, beta, pr, py, C, HW, slope);
            else
                hipLaunchKernelGGL((bn_act_fwd_kernel<ACT, false>), dim3((HW + 255) / 256, nb * Cy), dim3(256), 0, stream, px, mean,
                                   invstd, gamma, beta, pr, py, C, HW, slope);
        });
    });
}

int mogan_bn_act_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, float* dx, float* dgamma, float* dbeta, int B, int C, int HW, int act,
                     float slope, int accumulate, void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW, act)) return MOGAN_ERR_SHAPE;
    if (!ws || ws_bytes < mogan_bn_ws_bytes(B, C, HW)) return MOGAN_ERR_WS;
    const Split s = make_split(B, C, HW);
    const int YS = s.bs * s.hs;
    if (YS > 65535) return MOGAN_ERR_SHAPE;
    if (bn_small_ok(B, C, HW))
        return launch_small_bwd(x, dy, mean, invstd, gamma, beta, dx, dgamma, dbeta, B, C, HW, act, slope, accumulate, 1, stream);
    const int Cy = act == MOGAN_ACT_GLU ? C / 2 : C;
    if (Cy > 65535) return MOGAN_ERR_SHAPE;
    double* part = (double*)ws;
    float* sums = (float*)((char*)ws + (size_t)C * YS * 4 * sizeof(double));
    const float inv_n = 1.f / ((float)B * (float)HW);
    return with_act(act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
        hipLaunchKernelGGL((bn_bwd_partial_kernel<ACT>), dim3(Cy, YS), dim3(256), 0, stream, x, dy, mean, invstd, gamma,
                           beta, B, C, HW, s, slope, part);
        if (bn_fused_ok(HW))                   // finalize folded into the apply pass: two launches
            return for_batch_chunks(B, Cy, [&](int b0, int nb) {
                hipLaunchKernelGGL((bn_bwd_apply_fused_kernel<ACT>), dim3((HW + FUSED_PER - 1) / FUSED_PER, nb * Cy), dim3(256), 0,
                                   stream, x + (size_t)b0 * C * HW, dy + (size_t)b0 * Cy * HW, mean, invstd, gamma, beta,
                                   (const double*)part, dx + (size_t)b0 * C * HW, dgamma, dbeta, C, HW, YS, slope, inv_n, accumulate,
                                   b0 == 0 ? 1 : 0);
            });
        hipLaunchKernelGGL((bn_bwd_finalize_kernel<ACT>), dim3((Cy + 255) / 256), dim3(256), 0, stream,
                           (const double*)part, C, YS, sums, dgamma, dbeta, accumulate);
        return for_batch_chunks(B, Cy, [&](int b0, int nb) {
            hipLaunchKernelGGL((bn_bwd_apply_kernel<ACT>), dim3((HW + 255) / 256, nb * Cy), dim3(256), 0, stream,
                               x + (size_t)b0 * C * HW, dy + (size_t)b0 * Cy * HW, mean, invstd, gamma, beta,
                               (const float*)sums, dx + (size_t)b0 * C * HW, C, HW, slope, inv_n);
        });
    });
}

int mogan_affine_act_fwd(const float* x, const float* scale, const float* shift, float* y, int B, int C, int HW,
                         int act, float slope, hipStream_t stream) {
    return affine_impl<false>(x, nullptr, scale, shift, y, B, C, HW, act, slope, stream);
}
int mogan_affine_act_bwd(const float* x, const float* dy, const float* scale, const float* shift, float* dx, int B,
                         int C, int HW, int act, float slope, hipStream_t stream) {
    return affine_impl<true>(x, dy, scale, shift, dx, B, C, HW, act, slope, stream);
}

// backward of y = relu(scale*conv + shift) given the OUTPUT y: dx = dy * scale[c] * (y > 0)
int mogan_affine_relu_bwd_out(const float* y, const float* dy, const float* scale, float* dx, int B, int C, int HW,
                              hipStream_t stream) {
    if (!bn_shape_ok(B, C, HW)) return MOGAN_ERR_SHAPE;
    const long long n = (long long)B * C * HW;
    hipLaunchKernelGGL(affine_relu_bwd_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, y, dy, scale, dx,
                       n, C, HW);
    return ok_launch();
}

}  // extern "C"
