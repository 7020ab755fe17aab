// mogan_adam.h -- the per-element arithmetic of the fused Adam (+EMA) step, written once (internal, like mogan_bn.h).
//
// adam_kernel (mogan_elem.hip: a flat bucket, four elements per thread) and wpack2_adam_kernel (mogan_pgemm.hip: one deep
// convolution weight, updated and packed in the same pass) differ in how they walk the memory, not in what they compute per
// element.  The library is built with -ffp-contract=off, so the operand order written here IS the update of both.
#ifndef MOGAN_ADAM_H
#define MOGAN_ADAM_H
#include <hip/hip_runtime.h>

// the scalars of one step.  step_size / inv_sqrt_bc2 come from the host's step count or, where the count lives on the
// device (dev_state, written by adam_prep_kernel), from dev_state[1] / dev_state[2]
struct AdamCoef { float beta1, beta2, eps, step_size, inv_sqrt_bc2, gscale, ema_decay; int eps_mode; };

__device__ __forceinline__ AdamCoef adam_coef(float beta1, float beta2, float eps, float step_size, float inv_sqrt_bc2,
                                              int eps_mode, float gscale, float ema_decay,
                                              const float* __restrict__ dev_state) {
    AdamCoef k;
    if (dev_state) { step_size = dev_state[1]; inv_sqrt_bc2 = dev_state[2]; }
    k.beta1 = beta1; k.beta2 = beta2; k.eps = eps; k.step_size = step_size; k.inv_sqrt_bc2 = inv_sqrt_bc2;
    k.gscale = gscale; k.ema_decay = ema_decay; k.eps_mode = eps_mode;
    return k;
}

// eps_mode 0: denom = sqrt(v) / sqrt(1 - b2^t) + eps;  1: denom = sqrt(v) + eps (the bias correction is in step_size).
// HAS_EMA: e <- ema_decay * e + (1 - ema_decay) * p_new, else e is left alone
template <bool HAS_EMA>
__device__ __forceinline__ void adam_update(const AdamCoef& k, float& p, float g, float& m, float& v, float& e) {
    const float gg = g * k.gscale;
    m = m * k.beta1 + (1.f - k.beta1) * gg;
    v = v * k.beta2 + (1.f - k.beta2) * gg * gg;
    const float denom = k.eps_mode == 0 ? (sqrtf(v) * k.inv_sqrt_bc2 + k.eps) : (sqrtf(v) + k.eps);
    p = p - k.step_size * (m / denom);
    if (HAS_EMA) e = e * k.ema_decay + (1.f - k.ema_decay) * p;
}

#endif
