// mogan_bn.h -- the arithmetic of training-mode BatchNorm + activation, written once (internal, like mogan_mma.h).
//
// mogan_norm.hip (one-, two-, three-launch and grouped kernels) and the deep-block tails of mogan_pgemm.hip differ in how
// they split the work over blocks and launches, not in what they compute per channel and per element; each of those
// formulas is one function here.  The library is built with -ffp-contract=off, so a formula gives the same bits wherever it
// is inlined: the operand order written here IS the arithmetic of every BatchNorm path.
//
// Conventions (nn.BatchNorm1d/2d in training mode): the normalisation uses the biased batch variance, clamped at 0, from
// fp64 sums; running_var receives the unbiased one; running <- (1 - momentum) * running + momentum * batch.
#ifndef MOGAN_BN_H
#define MOGAN_BN_H
#include <hip/hip_runtime.h>
#include "../../include/mogan_hip.h"

__device__ __forceinline__ float bn_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }

template <int ACT>
__device__ __forceinline__ float act_fwd(float t, float slope) {
    if (ACT == MOGAN_ACT_RELU) return t > 0.f ? t : 0.f;
    if (ACT == MOGAN_ACT_LRELU) return t > 0.f ? t : t * slope;
    return t;
}

// a channel's normalisation: xhat = (x - mu) * is, BN output = x * sc + sh
struct BnCoef { float mu, is, sc, sh; };

__device__ __forceinline__ BnCoef bn_coef(float mu, float is, const float* __restrict__ gamma, const float* __restrict__ beta,
                                          int c) {
    BnCoef k;
    k.mu = mu; k.is = is;
    k.sc = gamma[c] * is; k.sh = beta[c] - mu * k.sc;
    return k;
}
__device__ __forceinline__ BnCoef bn_coef(const float* __restrict__ mean, const float* __restrict__ invstd,
                                          const float* __restrict__ gamma, const float* __restrict__ beta, int c) {
    return bn_coef(mean[c], invstd[c], gamma, beta, c);
}
// channel c and, for GLU, its gate channel c + Cy (zeros otherwise)
template <int ACT>
__device__ __forceinline__ void bn_coef_pair(const float* __restrict__ mean, const float* __restrict__ invstd,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, int c, int Cy,
                                             BnCoef& a, BnCoef& g) {
    a = bn_coef(mean, invstd, gamma, beta, c);
    g = BnCoef{0.f, 0.f, 0.f, 0.f};
    if (ACT == MOGAN_ACT_GLU) g = bn_coef(mean, invstd, gamma, beta, c + Cy);
}

__device__ __forceinline__ float bn_xhat(const BnCoef& k, float x) { return (x - k.mu) * k.is; }

// ------------------------------------------------------------------------------------------------ statistics
__device__ __forceinline__ void bn_stats_of(double sum, double sumsq, double n, float eps, float& mean, float& invstd,
                                            double& var) {
    const double m = sum / n;
    var = sumsq / n - m * m; if (var < 0) var = 0;
    mean = (float)m; invstd = (float)(1.0 / sqrt(var + (double)eps));
}
__device__ __forceinline__ double bn_unbiased(double var, double n) { return n > 1 ? var * n / (n - 1.0) : var; }
__device__ __forceinline__ float bn_running_mix(float running, float batch, float momentum) {
    return (1.f - momentum) * running + momentum * batch;
}
// one BatchNorm call's update of channel c (var: the biased batch variance; either buffer may be NULL)
__device__ __forceinline__ void bn_running_update(float* __restrict__ rmean, float* __restrict__ rvar, int c, float mean,
                                                  double var, double n, float momentum) {
    if (rmean) rmean[c] = bn_running_mix(rmean[c], mean, momentum);
    if (rvar) rvar[c] = bn_running_mix(rvar[c], (float)bn_unbiased(var, n), momentum);
}

// ------------------------------------------------------------------------------------------------ forward, one element
// xa: the channel's value, xg: the GLU gate channel's (unused otherwise); the residual is added by the caller
template <int ACT>
__device__ __forceinline__ float bn_fwd_elem(float xa, float xg, const BnCoef& a, const BnCoef& g, float slope) {
    const float t = xa * a.sc + a.sh;
    if (ACT == MOGAN_ACT_GLU) return t * bn_sigmoid(xg * g.sc + g.sh);
    return act_fwd<ACT>(t, slope);
}

// ------------------------------------------------------------------------------------------------ backward, one element
// dy (gradient at the activation output) -> da, dg (gradients at the BN outputs), recomputing the BN output from x.
// Non-GLU: channel c only (dg = 0).  GLU: pair (c, c+Cy): a = bn_c, g = bn_{c+Cy}; y = a*sig(g).
template <int ACT>
__device__ __forceinline__ void act_bwd(float xa, float xg, float dyv, const BnCoef& a, const BnCoef& g, float slope,
                                        float& da, float& dg) {
    if (ACT == MOGAN_ACT_GLU) {
        const float av = xa * a.sc + a.sh, s = bn_sigmoid(xg * g.sc + g.sh);
        da = dyv * s; dg = dyv * av * s * (1.f - s);
    } else {
        const float t = xa * a.sc + a.sh;
        if (ACT == MOGAN_ACT_RELU) da = t > 0.f ? dyv : 0.f;
        else if (ACT == MOGAN_ACT_LRELU) da = t > 0.f ? dyv : dyv * slope;
        else da = dyv;
        dg = 0.f;
    }
}
// acc += [da, da*xhat_a, dg, dg*xhat_g]: the two reductions of the BN backward (per half of a GLU pair)
template <int ACT>
__device__ __forceinline__ void bn_bwd_accum(double (&acc)[4], float xa, float xg, float dyv, const BnCoef& a, const BnCoef& g,
                                             float slope) {
    float da, dg;
    act_bwd<ACT>(xa, xg, dyv, a, g, slope, da, dg);
    acc[0] += da; acc[1] += (double)da * bn_xhat(a, xa);
    if (ACT == MOGAN_ACT_GLU) { acc[2] += dg; acc[3] += (double)dg * bn_xhat(g, xg); }
}
// dx = gamma*invstd * (dy_bn - sum_dy/n - xhat * sum_dyxhat/n)
__device__ __forceinline__ float bn_dx(float sc, float d, float xhat, float sum_d, float sum_dxhat, float inv_n) {
    return sc * (d - sum_d * inv_n - xhat * sum_dxhat * inv_n);
}
// s = the channel pair's four sums as bn_bwd_accum orders them; og is 0 without GLU
template <int ACT>
__device__ __forceinline__ void bn_bwd_elem(float xa, float xg, float dyv, const BnCoef& a, const BnCoef& g, float slope,
                                            const float (&s)[4], float inv_n, float& oa, float& og) {
    float da, dg;
    act_bwd<ACT>(xa, xg, dyv, a, g, slope, da, dg);
    oa = bn_dx(a.sc, da, bn_xhat(a, xa), s[0], s[1], inv_n);
    og = (ACT == MOGAN_ACT_GLU) ? bn_dx(g.sc, dg, bn_xhat(g, xg), s[2], s[3], inv_n) : 0.f;
}
// d beta = sum dy_bn, d gamma = sum dy_bn*xhat; accumulate: add to what the buffers hold (either may be NULL)
__device__ __forceinline__ void bn_write_dparam(float* __restrict__ dgamma, float* __restrict__ dbeta, int c, float sum_d,
                                                float sum_dxhat, int accumulate) {
    if (dbeta) dbeta[c] = (accumulate ? dbeta[c] : 0.f) + sum_d;
    if (dgamma) dgamma[c] = (accumulate ? dgamma[c] : 0.f) + sum_dxhat;
}
#endif
