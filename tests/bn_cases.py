"""Shapes, inputs, fp64 references and per-element bounds of the batch-norm / affine / activation / bias entry points of
include/mogan_hip.h (a plain helper module, not a conftest, like tests/conv_cases.py).  tests/test_bn_entry_points_gpu.py runs
the table through the C ABI under tests/memguard.py; tests/test_bn_reference_cpu.py keeps the references equal to
F.batch_norm in fp64, derives the TOL_* constants below from two fp32 CPU evaluations, holds the affine / activation / bias
bounds against fp32 evaluations of those kernels' formulas and asserts the kink condition and the path coverage.  Nothing here needs a GPU or the library.

Paths, restated from the words of include/mogan_hip.h / the head of csrc/mogan_norm.hip (not read from the library):
    one launch      HW >= 16 and B*HW <= 4096
    two launches    HW % 4 == 0 and HW >= 64
    three launches  everything else; HW == 1 (BatchNorm1d) takes the thread-per-channel statistics kernel
    batch chunks    the apply grids carry (image, channel) in a grid extent of 65535: B * Cy beyond that goes out in chunks

Bounds.  |got - fp64| <= TOL[kind] * S + F, per element.  S is the first-order sum over the absolute terms of what an fp32
evaluation of the formula can lose, the rounding of the fp32 statistics it consumes included; F is what does not scale with the
arithmetic's quality: a fixed number of fp32 roundings of an fp64 value (mean, invstd, the running statistics, d gamma / d beta
as rounded fp64 sums).  With sc = gamma * invstd:
    S_xhat = (|x| + |mean|) * invstd
    S_y    = |sc| * (|x| + |mean|) + |beta| (+ |res|)         (x*sc + sh with sh = beta - mean*sc, not (x - mean)*sc)
    sigmoid(g) of a BN output g: S_sig = s(1-s) * (S_g + 2 + |g|) + 3s.  The kernels' sigmoid is 1 / (1 + __expf(-g)), and __expf is
           v_exp_f32 of the fp32-rounded product g * log2(e): the instruction is documented to 1 ulp (2^-23 relative), the rounded
           product adds 2^-24 * |g| relative: together what a perturbation of the argument by 2^-24 * (2 + |g|) does; 1 + e, the
           division and the product with a are three more roundings.  These terms are counted in units of 2^-24 and scaled by TOL,
           which test_bn_reference_cpu asserts to be >= 2^-24: the documented accuracy is added, not fitted.
    GLU    S_y = S_a * s + |a| * S_sig + |a| * s
    d      the gradient at the BN output: exact for NONE / RELU (a select), one rounding for LRELU, for GLU
           da = dy * s: E = |dy| * (S_sig + s);  dg = dy * a * s * (1-s): E = |dy| * (S_a * s(1-s) + |a| * |1-2s| * S_sig + 4 |a| s(1-s))
    S_dx   = |sc| * (|d| + E + (|s0| + sum_j E_j) / n + S_xhat * |s1| / n + |xhat| * (|s1| + sum_j (|d_j| * S_xhat_j + E_j * |xhat_j|)) / n)
           (s0 = sum d, s1 = sum d * xhat; the last term is the error s1 inherits from the rounded mean and invstd)
    d beta, d gamma: F = 2^-24 * |sum| (G groups: once per group and once per addition), S = the sums of the terms' own S:
           of |d_j| + E_j and of |d_j| * S_xhat_j + E_j * |xhat_j|
    mean   F = 2^-24 * |mean| + D * 2^-53 * E|x|
    invstd F = 2^-24 * invstd + invstd^3 / 2 * dvar, dvar = 2 * D * 2^-53 * (E[x^2] + mean^2): the reference takes the variance
           from the centred values, the kernels from E[x^2] - mean^2 in fp64, whose two fp64 sums each lose at most D * 2^-53 of the
           sum of their absolute terms.  D = n / 256 + 80: the longest chain of additions a value of the sum passes through -- a
           thread's share of the channel, the wave and block trees (6 + 2), the partial slabs of the channel (a few dozen here).
    running statistics: F = 3 * 2^-24 * (|(1-m) r| + |m batch|) + m * (the batch statistic's own F); the unbiased variance is
           one more fp32 rounding of an fp64 value.  The reference multiplies with the fp32 values of momentum and of 1 - momentum.

The large-offset channel (|mean| / std about 1e3) makes S_y about 1e3 times the size of the values: no input keeps the sign of a
pre-activation safe against an error of that size, so that channel exists in the inputs of NONE and GLU only (kind_of).  Everywhere
else RELU / LRELU inputs keep |pre-activation| >= KINK * TOL["y"] * S_y: where det_array puts a value closer, the builder moves
that x by KINK_STEP (at most a handful of elements of a row; the CPU module asserts the condition on what the builder returns).
"""
import functools
import math

import numpy as np
import torch

from helpers import det_array

NONE, RELU, LRELU, GLU, TANH, SIGMOID = 0, 1, 2, 3, 4, 5
ACT_NAMES = {NONE: "none", RELU: "relu", LRELU: "lrelu", GLU: "glu", TANH: "tanh", SIGMOID: "sigmoid"}
BN_ACTS = (NONE, RELU, LRELU, GLU)
# the fp32 values the entry points receive, as the fp64 numbers the references compute with
SLOPE = float(np.float32(0.2))
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
ONE_MINUS_MOM = float(np.float32(1.0) - np.float32(0.1))      # (1.f - momentum) as the kernels form it
EPS32 = 2.0 ** -24
U64 = 2.0 ** -53
TOL_CEILING = 1e-5            # conv_cases.TOL_CEILING
KINK = 16.0
KINK_STEP = 1.0 / 32
CONST_VALUE = 0.75
OFFSET = 1000.0

# Per-element tolerances: 4 x the largest (err - F) / S of two fp32 CPU evaluations over every row and activation of the tables
# below (tests/test_bn_reference_cpu.py measures both, asserts the factor 4 and the ceiling, and prints the figures).  Measured, in
# units of 2^-24:
#     the restatement of csrc/mogan_bn.h in numpy fp32 (restate_fp32: operand order kept, fp64 sums)   y 3.18   dx 3.78   d gamma / d beta 0.86
#     torch's own fp32 CPU batch_norm, forward and backward                                            y 3.46   dx 48.79  d gamma / d beta 1.44
# y and the parameter gradients take the larger of the two.  dx does not: torch's backward sums a channel in fp32, and S_dx is written
# for the fp64 sums of the header (|s0| / n, not sum |d| / n), so where |d| and |xhat| are small torch's summation noise is all there
# is, and 4 x 48.79 x 2^-24 = 1.2e-5 would be above the ceiling.  That figure is a finding about the yardstick, recorded here and
# printed by the CPU module; TOL["dx"] is 4 x the restatement's, the tighter of the two.
TOL = {"y": 8.3e-7, "dx": 9.1e-7, "dparam": 3.5e-7}
MEASURED = {"y": 3.47 * EPS32, "dx": 3.80 * EPS32, "dparam": 1.45 * EPS32}

# ------------------------------------------------------------------------------------------------------------------ tables
ONE_LAUNCH = [(1, 2, 4, 4), (4, 8, 8, 8), (3, 6, 15, 15), (16, 6, 16, 16)]
TWO_LAUNCH = [(17, 6, 16, 16), (2, 4, 41, 100)]
BIG_TWO_LAUNCH = {NONE: (66, 1010, 8, 8), RELU: (66, 1010, 8, 8), LRELU: (66, 1010, 8, 8), GLU: (66, 2020, 8, 8)}
THREE_LAUNCH = [(20, 4, 15, 15), (5, 4, 3, 3), (130, 3, 6, 6), (34, 2000, 3, 3)]
BN1D = [(16, 24), (5, 300), (1, 3)]
GROUPED = [(3, 2, 4, 4, 4), (2, 16, 8, 16, 16), (2, 5, 10)]
GROUPED_INELIGIBLE = (3, 32, 4, 16, 16)
AFFINE = [(3, 6, 5, 7), (66, 1000, 3, 3)]
GLU_C2 = (3, 2, 5, 7)

BN_ROWS = [(s, a) for s in ONE_LAUNCH + TWO_LAUNCH for a in BN_ACTS] + [(BIG_TWO_LAUNCH[a], a) for a in BN_ACTS] \
    + [(s, a) for s in THREE_LAUNCH + BN1D for a in BN_ACTS]
BN_ROWS = [(s, a) for s, a in BN_ROWS if not (a == GLU and s[1] % 2)]       # (GLU halves the channels: an odd C is a rejection)
# the calls of the fused forward and of the backward, (shape, activation, residual): the residual rides on NONE, once per path
RES_SHAPES = (ONE_LAUNCH[2], TWO_LAUNCH[1], THREE_LAUNCH[0])
BN_CALLS = [(s, a, r) for s, a in BN_ROWS for r in ((False, True) if a == NONE and s in RES_SHAPES else (False,))]


def dims(shape):
    """(B, C, HW) of a (B, C, spatial...) shape"""
    return shape[0], shape[1], int(np.prod(shape[2:], dtype=np.int64))


def path_of(shape):
    B, C, HW = dims(shape)
    if HW >= 16 and B * HW <= 4096:
        return "one"
    if HW % 4 == 0 and HW >= 64:
        return "two"
    return "three"


def stats_kernel(shape):
    return "per-channel-thread" if dims(shape)[2] == 1 else "per-slab-block"


def chunks(shape, act):
    """the batch ranges the apply launches of the two- and three-launch paths cover"""
    B, C, HW = dims(shape)
    per = 65535 // (C // 2 if act == GLU else C)
    return [min(per, B - b0) for b0 in range(0, B, per)]


def T(name, shape, scale=1.0, shift=0.0):
    return torch.from_numpy(det_array(name, shape, scale, shift))


def kind_of(act):
    """which inputs an activation runs on: "lin" (NONE, GLU: with the large-offset channel) or "kink" (RELU, LRELU)"""
    return "lin" if act in (NONE, GLU) else "kink"


# ------------------------------------------------------------------------------------------------------------------ fp64
def _c(v):
    return v.view(1, -1, 1)


def sigmoid_parts(g, S_g):
    s = torch.sigmoid(g)
    return s, s * (1 - s) * (S_g + 2 + g.abs()) + 3 * s


def bn_forward(x, gamma, beta, act, res=None, rm=None, rv=None, mean=None, invstd=None, one_minus=ONE_MINUS_MOM):
    """fp64 training-mode BatchNorm + activation (+ residual) of x (B, C, HW); mean / invstd given: the apply half alone.
    -> ref, S, F (dicts over mean, invstd, y, rm, rv) and ctx for bn_backward"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    B, C, HW = x.shape
    n = B * HW
    ref, S, Fx = {}, {}, {}
    if mean is None:
        mean = x.mean((0, 2))
        var = ((x - _c(mean)) ** 2).mean((0, 2)).clamp_min(0)
        invstd = 1.0 / torch.sqrt(var + EPS)
        D = n / 256.0 + 80
        ex, ex2 = x.abs().mean((0, 2)), (x * x).mean((0, 2))
        dvar = 2 * D * U64 * (ex2 + mean * mean)
        ref["mean"], Fx["mean"] = mean, EPS32 * mean.abs() + D * U64 * ex
        ref["invstd"], Fx["invstd"] = invstd, EPS32 * invstd + 0.5 * invstd ** 3 * dvar
        unb = var * n / (n - 1.0) if n > 1 else var
        F_unb = EPS32 * unb + dvar * (n / (n - 1.0) if n > 1 else 1.0)
        for key, run, batch, Fb in (("rm", rm, mean, Fx["mean"]), ("rv", rv, unb, F_unb)):
            if run is not None:
                r = run.double()
                ref[key] = one_minus * r + MOM * batch
                Fx[key] = 3 * EPS32 * ((one_minus * r).abs() + (MOM * batch).abs()) + MOM * Fb
    else:
        mean, invstd = mean.double(), invstd.double()
    sc = gamma * invstd
    t = x * _c(sc) + _c(beta - mean * sc)
    S_t = _c(sc.abs()) * (x.abs() + _c(mean.abs())) + _c(beta.abs())
    ctx = dict(x=x, mean=mean, invstd=invstd, sc=sc, t=t, S_t=S_t, act=act, n=n)
    if act == GLU:
        Cy = C // 2
        a, g, S_a, S_g = t[:, :Cy], t[:, Cy:], S_t[:, :Cy], S_t[:, Cy:]
        s, S_sig = sigmoid_parts(g, S_g)
        y, S_y = a * s, S_a * s + a.abs() * S_sig + (a * s).abs()
        ctx.update(a=a, s=s, S_a=S_a, S_sig=S_sig)
    elif act == RELU:
        y, S_y = t.clamp_min(0), S_t
    elif act == LRELU:
        y, S_y = torch.where(t > 0, t, t * SLOPE), S_t
    else:
        y, S_y = t, S_t
    if res is not None:
        y, S_y = y + res.double(), S_y + res.double().abs()
    ref["y"], S["y"] = y, S_y
    return ref, S, Fx, ctx


def bn_backward(ctx, dy, ngroups_rounded=1):
    """fp64 gradients of bn_forward at dy (B, Cy, HW) -> ref, S, F over dx, dgamma, dbeta"""
    x, mean, invstd, sc, t, act, n = (ctx[k] for k in ("x", "mean", "invstd", "sc", "t", "act", "n"))
    dy = dy.double()
    xhat = (x - _c(mean)) * _c(invstd)
    S_xhat = (x.abs() + _c(mean.abs())) * _c(invstd)
    if act == GLU:
        a, s, S_a, S_sig = (ctx[k] for k in ("a", "s", "S_a", "S_sig"))
        d = torch.cat([dy * s, dy * a * s * (1 - s)], 1)
        E = torch.cat([dy.abs() * (S_sig + s),
                       dy.abs() * (S_a * s * (1 - s) + a.abs() * (1 - 2 * s).abs() * S_sig + 4 * a.abs() * s * (1 - s))], 1)
    elif act == RELU:
        d, E = torch.where(t > 0, dy, torch.zeros_like(dy)), torch.zeros_like(dy)
    elif act == LRELU:
        d = torch.where(t > 0, dy, dy * SLOPE)
        E = torch.where(t > 0, torch.zeros_like(dy), d.abs())
    else:
        d, E = dy, torch.zeros_like(dy)
    s0, s1 = d.sum((0, 2)), (d * xhat).sum((0, 2))
    A0 = E.sum((0, 2))
    D0 = d.abs().sum((0, 2))
    A1 = (d.abs() * S_xhat + E * xhat.abs()).sum((0, 2))
    ref = {"dx": _c(sc) * (d - _c(s0) / n - xhat * _c(s1) / n), "dbeta": s0, "dgamma": s1}
    S = {"dx": _c(sc.abs()) * (d.abs() + E + _c(s0.abs() + A0) / n + S_xhat * _c(s1.abs()) / n + xhat.abs() * _c(s1.abs() + A1) / n),
         "dbeta": D0 + A0, "dgamma": A1}
    Fx = {"dbeta": ngroups_rounded * EPS32 * s0.abs(), "dgamma": ngroups_rounded * EPS32 * s1.abs()}
    return ref, S, Fx


def bound(key, S, Fx, base=None):
    """TOL * S + F of one output (+ 2 * 2^-24 * (|base| + S + |F / 2^-24|) when the entry point adds into `base`)"""
    tol = TOL["y" if key == "y" else "dx" if key == "dx" else "dparam"]
    b = tol * S.get(key, 0.0) + Fx.get(key, 0.0)
    if base is not None:
        b = b + 2 * EPS32 * (base.double().abs() + S.get(key, 0.0) + Fx.get(key, 0.0) / EPS32)
    return b


# --------------------------------------------------------------------------------------------------------------- inputs
def _special_channels(x, C, kind):
    """channel 0 constant; the last channel on a large offset where the activation has no kink"""
    x[:, 0] = CONST_VALUE
    if kind == "lin":
        x[:, C - 1] = (x[:, C - 1].double() / 1.5 + OFFSET).float()
    return x


def _unkink(x, gamma, beta, groups=1):
    """move the x whose fp64 pre-activation lies within KINK * TOL * S_y of 0 by KINK_STEP; -> how many were moved"""
    moved = 0
    per = x.shape[0] // groups
    for g in range(groups):
        xs = x[g * per:(g + 1) * per]
        for _ in range(4):                              # (a moved value shifts the channel's statistics a little)
            _, _, _, ctx = bn_forward(xs, gamma, beta, NONE)
            near = ctx["t"].abs() < KINK * TOL["y"] * ctx["S_t"]
            near[:, 0] = False                          # (the constant channel sits at beta: see bn_inputs)
            if not bool(near.any()):
                break
            xs[near] += KINK_STEP
            moved += int(near.sum())
    return moved


@functools.lru_cache(maxsize=None)
def bn_inputs(shape, kind, groups=1):
    """x (groups*B, C, HW), gamma, beta, running_mean, running_var (fp32 tensors) of a row.  beta of the constant channel is
    +-0.25: its pre-activation IS beta (x = mean), so no step on x could move it off a kink (n = 1: every channel's)."""
    B, C, HW = dims(shape)
    tag = "%s%s%d" % (shape, kind, groups)
    x = _special_channels(T("bnx" + tag, (groups * B, C, HW), 1.5, 0.3), C, kind)
    gamma, beta = T("bng" + tag, (C,), 0.2, 1.0), T("bnb" + tag, (C,), 0.2)
    beta[0] = 0.25 if C % 4 else -0.25
    if B * HW == 1:                                     # n = 1: every channel is constant
        beta[:] = torch.tensor([0.25, -0.25] * C)[:C]
    d = dict(x=x, gamma=gamma, beta=beta, rm=T("bnrm" + tag, (C,), 0.1), rv=T("bnrv" + tag, (C,), 0.1).abs() + 1, moved=0)
    if kind == "kink":
        d["moved"] = _unkink(x, gamma, beta, groups)
    return d


def bn_dy(shape, act, groups=1):
    B, C, HW = dims(shape)
    return T("bndy%s%d%d" % (shape, act, groups), (groups * B, C // 2 if act == GLU else C, HW))


def bn_res(shape):
    return T("bnres%s" % (shape,), dims(shape))


def grouped_reference(x, gamma, beta, act, rm, rv, dy, G):
    """G calls in sequence on the G groups of x: per-group statistics (G x C), running statistics updated group after group,
    parameter gradients summed -> ref, bounds (already TOL * S + F) over mean, invstd, y, rm, rv, dx, dgamma, dbeta"""
    per = x.shape[0] // G
    parts = {k: [] for k in ("mean", "invstd", "y", "dx")}
    bparts = {k: [] for k in parts}
    ref, bnd = {}, {}
    for g in range(G):
        sl = slice(g * per, (g + 1) * per)
        r, S, Fx, ctx = bn_forward(x[sl], gamma, beta, act, None, rm, rv)
        for k in ("mean", "invstd", "y"):
            parts[k].append(r[k]); bparts[k].append(bound(k, S, Fx))
        # the running statistics carry the earlier groups' error on, scaled by 1 - momentum
        for k in ("rm", "rv"):
            bnd[k] = bound(k, S, Fx) + (ONE_MINUS_MOM * bnd[k] if k in bnd else 0.0)
            ref[k] = r[k]
        rm, rv = r["rm"], r["rv"]
        rb, Sb, Fb = bn_backward(ctx, dy[sl], 2)
        parts["dx"].append(rb["dx"]); bparts["dx"].append(bound("dx", Sb, Fb))
        for k in ("dgamma", "dbeta"):
            ref[k] = ref.get(k, 0.0) + rb[k]
            bnd[k] = bnd.get(k, 0.0) + bound(k, Sb, Fb)
    for k in ("mean", "invstd"):
        ref[k], bnd[k] = torch.stack(parts[k]), torch.stack(bparts[k])
    for k in ("y", "dx"):
        ref[k], bnd[k] = torch.cat(parts[k]), torch.cat(bparts[k])
    return ref, bnd


# ------------------------------------------------------------------------------------------- affine / activation / bias
def affine_inputs(shape, act):
    """x (B, C, HW), scale, shift, dy; RELU / LRELU: no pre-activation within KINK * TOL * S of 0 (moved by KINK_STEP)"""
    B, C, HW = dims(shape)
    x = T("afx%s" % (shape,), (B, C, HW), 1.5, 0.3)
    scale, shift = T("afs%d" % C, (C,), 0.5, 1.0), T("afb%d" % C, (C,), 0.3)
    moved = 0
    if act in (RELU, LRELU):
        ref, S, _ = affine_reference(x, scale, shift, NONE)
        near = ref["y"].abs() < KINK * TOL["y"] * S["y"]
        x[near] += KINK_STEP
        moved = int(near.sum())
    return dict(x=x, scale=scale, shift=shift, dy=T("afg%s%d" % (shape, act), (B, C, HW)), moved=moved)


def affine_reference(x, scale, shift, act, dy=None):
    """y = act(x * scale + shift), dx = dy * act' * scale -> ref, S, F"""
    x, scale, shift = x.double(), _c(scale.double()), _c(shift.double())
    t = x * scale + shift
    ref = {"y": t.clamp_min(0) if act == RELU else torch.where(t > 0, t, t * SLOPE) if act == LRELU else t}
    S = {"y": (x * scale).abs() + shift.abs()}
    Fx = {}
    if dy is not None:
        d = dy.double()
        d = torch.where(t > 0, d, torch.zeros_like(d)) if act == RELU else torch.where(t > 0, d, d * SLOPE) if act == LRELU else d
        ref["dx"] = d * scale
        Fx["dx"] = 2 * EPS32 * ref["dx"].abs()          # d * slope, * scale: two roundings
    return ref, S, Fx


def act_reference(x, act, dy):
    """mogan_act_fwd / _bwd on x (B, C, HW) -> ref, F (absolute bounds) over y, dx.  RELU / LRELU select on the sign of the fp32
    input itself: exact, one rounding for the slope.  SIGMOID / GLU: the fast exponential as in the module docstring (S_g = 0: the
    argument is an input).  TANH is tanhf of the device library, documented to 2 ulp: 4 * 2^-24 * |tanh|."""
    x, dy = x.double(), dy.double()
    if act in (RELU, LRELU):
        k = 0.0 if act == RELU else SLOPE
        y, dx = torch.where(x > 0, x, x * k), torch.where(x > 0, dy, dy * k)
        return {"y": y, "dx": dx}, {"y": EPS32 * y.abs(), "dx": EPS32 * dx.abs()}
    if act == TANH:
        t = torch.tanh(x)
        Ft = 4 * EPS32 * t.abs()
        dx = dy * (1 - t * t)
        return {"y": t, "dx": dx}, {"y": Ft, "dx": dy.abs() * (2 * t.abs() * Ft + 3 * EPS32 * (1 + t * t))}
    if act == SIGMOID:
        s, S_sig = sigmoid_parts(x, 0.0)
        dx = dy * s * (1 - s)
        return {"y": s, "dx": dx}, {"y": EPS32 * S_sig, "dx": EPS32 * dy.abs() * ((1 - 2 * s).abs() * S_sig + 4 * s * (1 - s))}
    Cy = x.shape[1] // 2
    a, g = x[:, :Cy], x[:, Cy:]
    s, S_sig = sigmoid_parts(g, 0.0)
    ref = {"y": a * s, "dx": torch.cat([dy * s, dy * a * s * (1 - s)], 1)}
    Fx = {"y": EPS32 * (a.abs() * S_sig + (a * s).abs()),
          "dx": EPS32 * torch.cat([dy.abs() * (S_sig + s), dy.abs() * a.abs() * ((1 - 2 * s).abs() * S_sig + 4 * s * (1 - s))], 1)}
    return ref, Fx


# ------------------------------------------------------------------------ the fp32 restatement of csrc/mogan_bn.h (numpy)
f32 = np.float32
LOG2E = f32(math.log2(math.e))


def _sig32(v):
    """1.f / (1.f + __expf(-v)) with a correctly rounded exp2 of the fp32-rounded product"""
    e = np.exp2((-v * LOG2E).astype(np.float64)).astype(f32)
    return f32(1) / (f32(1) + e)


def restate_fp32(x, gamma, beta, act, res, dy, rm, rv):
    """mogan_bn.h in its operand order, one fp32 rounding per operation, fp64 sums: bn_stats_of, bn_coef (sc = gamma * is,
    sh = beta - mu * sc), bn_fwd_elem (t = x * sc + sh), act_bwd, bn_bwd_accum, bn_dx, bn_running_update.  numpy fp32 arrays
    (B, C, HW) / (C,) -> dict over mean, invstd, y, rm, rv, dx, dgamma, dbeta"""
    B, C, HW = x.shape
    n = float(B * HW)
    c = lambda v: v.reshape(1, -1, 1)
    x64 = x.astype(np.float64)
    m = x64.sum((0, 2)) / n
    var = np.maximum((x64 * x64).sum((0, 2)) / n - m * m, 0.0)
    mu, is_ = m.astype(f32), (1.0 / np.sqrt(var + EPS)).astype(f32)
    out = {"mean": mu, "invstd": is_}
    mom, eps = f32(0.1), f32(1e-5)
    unb = (var * n / (n - 1.0) if n > 1 else var).astype(f32)
    out["rm"] = (f32(1) - mom) * rm + mom * mu
    out["rv"] = (f32(1) - mom) * rv + mom * unb
    sc = gamma * is_
    sh = beta - mu * sc
    t = x * c(sc) + c(sh)
    slope = f32(0.2)
    Cy = C // 2
    if act == GLU:
        s = _sig32(t[:, Cy:])
        y = t[:, :Cy] * s
    elif act == RELU:
        y = np.where(t > 0, t, f32(0))
    elif act == LRELU:
        y = np.where(t > 0, t, t * slope)
    else:
        y = t
    out["y"] = y + res if res is not None else y
    if act == GLU:
        av = t[:, :Cy]
        d = np.concatenate([dy * s, dy * av * s * (f32(1) - s)], 1)
    elif act == RELU:
        d = np.where(t > 0, dy, f32(0))
    elif act == LRELU:
        d = np.where(t > 0, dy, dy * slope)
    else:
        d = dy
    xhat = (x - c(mu)) * c(is_)
    s0 = d.astype(np.float64).sum((0, 2)).astype(f32)
    s1 = (d.astype(np.float64) * xhat).sum((0, 2)).astype(f32)
    inv_n = f32(1) / (f32(B) * f32(HW))
    out["dx"] = c(sc) * (d - c(s0) * inv_n - xhat * c(s1) * inv_n)
    out["dbeta"], out["dgamma"] = s0, s1
    assert all(v.dtype == f32 for v in out.values())
    return out


def restate_affine_fp32(x, scale, shift, act, dy):
    """affine_act_kernel: bn_fwd_elem / act_bwd with sc = scale, sh = shift; dx = d * sc.  numpy fp32 -> dict over y, dx"""
    c = lambda v: v.reshape(1, -1, 1)
    slope = f32(0.2)
    t = x * c(scale) + c(shift)
    y = np.where(t > 0, t, f32(0)) if act == RELU else np.where(t > 0, t, t * slope) if act == LRELU else t
    d = np.where(t > 0, dy, f32(0)) if act == RELU else np.where(t > 0, dy, dy * slope) if act == LRELU else dy
    out = {"y": y, "dx": d * c(scale)}
    assert all(v.dtype == f32 for v in out.values())
    return out


def restate_act_fp32(x, act, dy):
    """act_kernel / glu_kernel of csrc/mogan_elem.hip in their operand order, one fp32 rounding per operation; the sigmoid as
    _sig32, tanh as numpy's own fp32 tanh (another library than the device's tanhf, held to the same documented 2 ulp)"""
    one, slope = f32(1), f32(0.2)
    if act in (RELU, LRELU):
        k = f32(0) if act == RELU else slope
        out = {"y": np.where(x > 0, x, x * k), "dx": np.where(x > 0, dy, dy * k)}
    elif act == TANH:
        t = np.tanh(x)
        out = {"y": t, "dx": dy * (one - t * t)}
    elif act == SIGMOID:
        s = _sig32(x)
        out = {"y": s, "dx": dy * s * (one - s)}
    else:
        Cy = x.shape[1] // 2
        a, s = x[:, :Cy], _sig32(x[:, Cy:])
        out = {"y": a * s, "dx": np.concatenate([dy * s, dy * a * s * (one - s)], 1)}
    assert all(v.dtype == f32 for v in out.values())
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def bn_case(shape, act, res=False):
    """inputs, fp64 references and S / F of one BatchNorm call on a row, computed once and shared by the tests (read-only)"""
    B, C, HW = dims(shape)
    inp = bn_inputs(shape, kind_of(act))
    dy = bn_dy(shape, act)
    r = bn_res(shape)[:, :C // 2 if act == GLU else C].contiguous() if res else None
    ref, S, Fx, ctx = bn_forward(inp["x"], inp["gamma"], inp["beta"], act, r, inp["rm"], inp["rv"])
    rb, Sb, Fb = bn_backward(ctx, dy)
    ref.update(rb); S.update(Sb); Fx.update(Fb)
    return dict(inp=inp, dy=dy, res=r, ref=ref, S=S, F=Fx, t=ctx["t"] if act in (RELU, LRELU) else None,
                S_t=ctx["S_t"] if act in (RELU, LRELU) else None)
